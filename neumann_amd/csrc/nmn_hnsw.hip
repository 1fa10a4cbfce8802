// nmn_hnsw.hip — `tensor_store::HNSWIndex` (tensor_store/src/hnsw.rs:1554-2335) with Dense storage: the graph is built on the
// host in the reference's order and searched on the GPU, one query per wave, the whole walk in one launch.
// THIS TRANSLATION UNIT IS BUILT WITH -ffp-contract=off -fhip-fp32-correctly-rounded-divide-sqrt (build.py), host and device:
// every distance below restates the reference's unfused f32 arithmetic and must give its bits.
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

#include "nmn_index.h"
#include "nmn_internal.h"
#include "nmn_hnsw_queue.h"
#include "nmn_tt.h"

#pragma clang fp contract(off)

namespace nmn {
namespace {

constexpr uint32_t kNone = 0xFFFFFFFFu;
constexpr uint32_t kLdsResultsMax = 1024;  // entries of the results heap a wave keeps in LDS (+1 for the push before the pop)
constexpr uint32_t kLdsCandMax = 4096;     // entries of the candidate heap a wave keeps in LDS
constexpr uint32_t kMaxDim = 8192;         // the query sits in LDS for the whole walk (32 KiB at most)
constexpr uint32_t kBulkMinRows = 4;       // rows a call must leave for the device to be walked there (the adaptive policy's smallest batch)
constexpr uint32_t kBulkMinNodes = 100000;  // the graph size from which the device walks by default: the measured break-even (docs/hnsw.md §19.5)
constexpr uint32_t kBulkBatchMax = 1024;   // nodes of one hnsw_insert_walk_kernel launch (nmn_hnsw_set_bulk_policy)
constexpr uint32_t kSparseLdsEntries = 4096;  // stored entries of a sparse query a wave keeps in LDS, 8 bytes each: the same 32 KiB

struct Ent {
    float d;
    uint32_t id;
};

// ---- the two heaps, shared by host and device ------------------------------------------------------------------------------
// MAX == true: MaxNeighbor (a <= b iff a.d <= b.d); MAX == false: Neighbor, reversed (a <= b iff b.d <= a.d).  NaN distances are out of scope.
template <bool MAX>
__host__ __device__ inline bool heap_le(const Ent& a, const Ent& b) {
    return MAX ? a.d <= b.d : b.d <= a.d;
}
// BinaryHeap::sift_up(start = 0, pos): the hole moves up while the element is GREATER than the parent
template <bool MAX>
__host__ __device__ inline void heap_sift_up(Ent* v, uint32_t pos) {
    const Ent e = v[pos];
    while (pos > 0) {
        const uint32_t parent = (pos - 1) / 2;
        if (heap_le<MAX>(e, v[parent])) break;
        v[pos] = v[parent];
        pos = parent;
    }
    v[pos] = e;
}
template <bool MAX>
__host__ __device__ inline void heap_push(Ent* v, uint32_t& n, Ent e) {
    v[n] = e;
    heap_sift_up<MAX>(v, n);
    n++;
}
// BinaryHeap::pop: Vec::pop, swap with the root, sift_down_to_bottom(0)
template <bool MAX>
__host__ __device__ inline Ent heap_pop(Ent* v, uint32_t& n) {
    Ent item = v[--n];
    if (n > 0) {
        const Ent root = v[0];
        const uint32_t end = n;
        uint32_t pos = 0, child = 1;
        while (child + 1 < end) {  // child <= end.saturating_sub(2)
            if (heap_le<MAX>(v[child], v[child + 1])) child++;
            v[pos] = v[child];
            pos = child;
            child = 2 * pos + 1;
        }
        if (child == end - 1) {
            v[pos] = v[child];
            pos = child;
        }
        v[pos] = item;
        heap_sift_up<MAX>(v, pos);
        item = root;
    }
    return item;
}

// ---- host arithmetic ---------------------------------------------------------------------------------------------------------
inline float h_dot8(const float* a, const float* b, uint32_t dim) {
    float acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    const uint32_t chunks = dim / 8;
    for (uint32_t c = 0; c < chunks; c++)
        for (int l = 0; l < 8; l++) {
            const float p = a[8 * c + l] * b[8 * c + l];
            acc[l] = acc[l] + p;
        }
    float r = -0.0f;
    for (int l = 0; l < 8; l++) r = r + acc[l];
    for (uint32_t i = chunks * 8; i < dim; i++) {
        const float p = a[i] * b[i];
        r = r + p;
    }
    return r;
}
inline float h_eucl8(const float* a, const float* b, uint32_t dim) {
    float acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    const uint32_t chunks = dim / 8;
    for (uint32_t c = 0; c < chunks; c++)
        for (int l = 0; l < 8; l++) {
            const float d = a[8 * c + l] - b[8 * c + l];
            const float p = d * d;
            acc[l] = acc[l] + p;
        }
    float r = -0.0f;
    for (int l = 0; l < 8; l++) r = r + acc[l];
    for (uint32_t i = chunks * 8; i < dim; i++) {
        const float d = a[i] - b[i];
        const float p = d * d;
        r = r + p;
    }
    return sqrtf(r);
}
inline float h_distance(int metric, const float* v, float vmag, const float* q, float qmag, uint32_t dim) {
    if (metric == NMN_METRIC_EUCLIDEAN) return h_eucl8(v, q, dim);
    const float dot = h_dot8(v, q, dim);
    if (metric == NMN_METRIC_DOT_PRODUCT) return -dot;
    if (vmag == 0.0f || qmag == 0.0f) return 1.0f;
    const float den = vmag * qmag;
    const float sim = dot / den;
    return 1.0f - sim;
}
__host__ __device__ inline float to_similarity(int metric, float d) {  // hnsw.rs:152-158
    if (metric == NMN_METRIC_EUCLIDEAN) return 1.0f / (1.0f + d);
    if (metric == NMN_METRIC_DOT_PRODUCT) return -d;
    return 1.0f - d;
}

// ---- ScalarQuantizedVector on the host (hnsw.rs:324-368, 414-527) ----------------------------------------------------------------
// from_dense: min / max by f32::min / f32::max folds, scale 1.0 when the range is below f32::EPSILON, round = half away from zero
inline void h_quantize(const float* v, uint32_t dim, uint8_t* code, float* scale_out, float* min_out) {
    float mn = INFINITY, mx = -INFINITY;
    for (uint32_t i = 0; i < dim; i++) {
        mn = fminf(mn, v[i]);
        mx = fmaxf(mx, v[i]);
    }
    const float range = mx - mn;
    const float scale = fabsf(range) < 1.1920928955078125e-07f ? 1.0f : range / 255.0f;
    for (uint32_t i = 0; i < dim; i++) {
        const float t = v[i] - mn;
        float r = roundf(t / scale);
        r = r < 0.0f ? 0.0f : (r > 255.0f ? 255.0f : r);
        code[i] = (uint8_t)r;
    }
    *scale_out = scale;
    *min_out = mn;
}
inline void h_dequantize(const uint8_t* code, uint32_t dim, float scale, float mn, float* out) {
    for (uint32_t i = 0; i < dim; i++) out[i] = __builtin_fmaf((float)code[i], scale, mn);
}
// the eight chains of `y` alone (sum_y of dot_dense: it depends on the query only)
inline float h_sum8(const float* y, uint32_t dim) {
    float acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    const uint32_t chunks = dim / 8;
    for (uint32_t c = 0; c < chunks; c++)
        for (int l = 0; l < 8; l++) acc[l] = acc[l] + y[8 * c + l];
    float r = -0.0f;
    for (int l = 0; l < 8; l++) r = r + acc[l];
    for (uint32_t i = chunks * 8; i < dim; i++) r = r + y[i];
    return r;
}
// dot_dense: q_dot_y in eight chains (product and sum rounded separately), then scale.mul_add(q_dot_y, min * sum_y)
inline float h_q8_dot(const uint8_t* code, float scale, float mn, const float* y, float sum_y, uint32_t dim) {
    float acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    const uint32_t chunks = dim / 8;
    for (uint32_t c = 0; c < chunks; c++)
        for (int l = 0; l < 8; l++) {
            const float p = (float)code[8 * c + l] * y[8 * c + l];
            acc[l] = acc[l] + p;
        }
    float r = -0.0f;
    for (int l = 0; l < 8; l++) r = r + acc[l];
    for (uint32_t i = chunks * 8; i < dim; i++) {
        const float p = (float)code[i] * y[i];
        r = r + p;
    }
    const float ms = mn * sum_y;
    return __builtin_fmaf(scale, r, ms);
}
// squared_magnitude: chains of q*q and q, then scale_sq.mul_add(sum_q_sq, ((2 scale) min).mul_add(sum_q, (min min) n))
inline float h_q8_sqmag(const uint8_t* code, float scale, float mn, uint32_t dim) {
    float a2[8] = {0, 0, 0, 0, 0, 0, 0, 0}, a1[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    const uint32_t chunks = dim / 8;
    for (uint32_t c = 0; c < chunks; c++)
        for (int l = 0; l < 8; l++) {
            const float q = (float)code[8 * c + l];
            const float p = q * q;
            a2[l] = a2[l] + p;
            a1[l] = a1[l] + q;
        }
    float s2 = -0.0f, s1 = -0.0f;
    for (int l = 0; l < 8; l++) s2 = s2 + a2[l];
    for (int l = 0; l < 8; l++) s1 = s1 + a1[l];
    for (uint32_t i = chunks * 8; i < dim; i++) {
        const float q = (float)code[i];
        const float p = q * q;
        s2 = s2 + p;
        s1 = s1 + q;
    }
    const float n = (float)dim;
    const float scale_sq = scale * scale;
    const float min_sq = mn * mn;
    const float two_s = 2.0f * scale;
    const float tsm = two_s * mn;
    const float msn = min_sq * n;
    const float inner = __builtin_fmaf(tsm, s1, msn);
    return __builtin_fmaf(scale_sq, s2, inner);
}
// what the query contributes to every distance, computed once: simd::magnitude (Cosine), sum_y (quantized rows), sum_of_squares
// (quantized rows under Euclidean)
struct HQ {
    float mag = 0.0f, sum = 0.0f, sq = 0.0f;
};
// EmbeddingStorage::distance_dense on a Quantized row (hnsw.rs:1035-1045 with magnitude_immutable 401-407; 522-527; 1136-1138)
inline float h_q8_distance(int metric, const uint8_t* code, float scale, float mn, float mag, float x_sq, const float* q, const HQ& hq,
                           uint32_t dim) {
    const float dot = h_q8_dot(code, scale, mn, q, hq.sum, dim);
    if (metric == NMN_METRIC_DOT_PRODUCT) return -dot;
    if (metric == NMN_METRIC_EUCLIDEAN) {
        const float s = x_sq + hq.sq;
        const float t = __builtin_fmaf(2.0f, -dot, s);
        return sqrtf(t > 0.0f ? t : 0.0f);  // `.max(0.0)`: NaN and negatives to 0.0
    }
    if (mag == 0.0f || hq.mag == 0.0f) return 1.0f;
    const float den = mag * hq.mag;
    const float sim = dot / den;
    return 1.0f - sim;
}

// ---- BinaryVector on the host (binary_quantization.rs:41-99, 123-166) -----------------------------------------------------------
// BinaryThreshold::compute: Sign 0.0; Mean `iter().sum::<f32>() / len as f32` (the fold from -0.0 of docs/hnsw.md §1); Median the
// sorted row's middle element, or f32::midpoint of the two middle ones = ((a as f64 + b as f64) / 2) as f32 (docs/ivf.md §3.10b).
// from_dense: bit i of word i / 64 = v[i] > threshold; the padding bits of the last word stay zero.  NaN rows are out of scope.
inline float h_bin_threshold(const float* v, uint32_t dim, int method, std::vector<float>& tmp) {
    if (method == NMN_BINARY_MEAN) {
        float s = -0.0f;
        for (uint32_t i = 0; i < dim; i++) s = s + v[i];
        return s / (float)dim;
    }
    if (method == NMN_BINARY_MEDIAN) {
        tmp.assign(v, v + dim);
        std::stable_sort(tmp.begin(), tmp.end());
        const uint32_t mid = dim / 2;
        if (dim % 2 == 0) return (float)(((double)tmp[mid - 1] + (double)tmp[mid]) / 2.0);
        return tmp[mid];
    }
    return 0.0f;
}
inline void h_bin_from_dense(const float* v, uint32_t dim, int method, uint64_t* words, float* pm1, std::vector<float>& tmp) {
    const float t = h_bin_threshold(v, dim, method, tmp);
    const uint32_t W = (dim + 63u) / 64u;
    for (uint32_t w = 0; w < W; w++) words[w] = 0;
    for (uint32_t i = 0; i < dim; i++) {
        const bool bit = v[i] > t;
        if (bit) words[i >> 6] |= 1ull << (i & 63u);
        pm1[i] = bit ? 1.0f : -1.0f;  // to_dense()
    }
}
inline uint32_t h_bin_hamming(const uint64_t* a, const uint64_t* b, uint32_t W) {
    uint32_t hd = 0;
    for (uint32_t w = 0; w < W; w++) hd += (uint32_t)__builtin_popcountll(a[w] ^ b[w]);
    return hd;
}
// EmbeddingStorage::distance_dense on a Binary row (hnsw.rs:1035-1045 with 801-805 and 981-984; 1098-1101; 1136-1138): `pm1` is
// to_dense(), sqrt_dim = (dimension as f32).sqrt(), the row's magnitude whatever its bits (never 0)
inline float h_bin_distance(int metric, const float* pm1, float sqrt_dim, const float* q, float qmag, uint32_t dim) {
    if (metric == NMN_METRIC_EUCLIDEAN) return h_eucl8(pm1, q, dim);
    const float dot = h_dot8(pm1, q, dim);
    if (metric == NMN_METRIC_DOT_PRODUCT) return -dot;
    if (qmag == 0.0f) return 1.0f;
    const float den = sqrt_dim * qmag;
    const float sim = dot / den;
    return 1.0f - sim;
}

// ---- device graph --------------------------------------------------------------------------------------------------------------
struct GraphDev {
    const float* corpus;    // the flat index's rows, stride ld
    const float* norms;     // simd::magnitude of every row (ingest kernels)
    const uint8_t* codes;   // quantized handle: the codes, stride ld8 (dim rounded up to 16, the padding zero); binary handle: the
                            // BinaryVector words, stride ld8 bytes (ceil(dim / 64) words rounded up to 2, the padding zero)
    const float4* rec;      // quantized handle: {scale, min_val, simd::magnitude(dequantize()), squared_magnitude()} per row
    const uint32_t* l0;     // [n][m0] layer-0 neighbour slots, id-ascending
    const uint32_t* l0cnt;  // [n]
    const uint32_t* up_idx; // [n] row of the upper table, kNone for a level-0 node
    const uint32_t* up;     // [n_upper][up_layers][m]
    const uint32_t* upcnt;  // [n_upper][up_layers]
    uint32_t ld, ld8, dim, m, m0, up_layers, n, entry, max_layer;
    int metric;
};

struct SearchArgs {
    GraphDev g;
    const float* queries;  // [nq][dim]
    uint32_t nq, k, ef;    // ef = max(ef, k) already
    uint32_t rcap, ccap;   // entries of the results / candidate heaps of this launch
    uint32_t qlds;         // query elements in LDS (dim rounded up to 8)
    uint32_t* visited;     // [nq][vwords]
    uint32_t vwords;
    uint32_t* flags;       // [nq] 0 = answered by the first launch, 1 = candidate heap overflowed, 2 = answered by the spill launch
    uint32_t* evals;       // [nq] distance evaluations
    Ent* spill;            // spill launch: [regions][rcap + ccap]
    uint64_t* out_ids;
    float* out_scores;
    uint32_t* out_counts;
    // hnsw_search_kernel<.., PERQ = true>: one k and one ef (= max(ef, k) already) per query of the launch, each array nullable
    // (null: k / ef above); kstride = row stride of out_ids / out_scores, the largest k of the launch.  ccap_fixed / the formula of
    // cand_cap() give every query the candidate limit it has in a launch of its own (rcap / ccap stay the launch's: the regions).
    const uint32_t* qk;
    const uint32_t* qef;
    uint32_t kstride, ccap_fixed;
    // hnsw_search_kernel<.., QK != 0> (nmn_hnsw_search_sparse, docs/hnsw.md §13).  QK == 1: query i is the stored entries
    // [sp_off[i], sp_off[i + 1]) of sp_ent, (position, value bits) pairs in SparseVector order, qlds / 2 of them at most; `queries`
    // is not read.  QK != 0: qmag[i] = SparseVector::magnitude() of query i, taken through f64 on the host.
    const uint64_t* sp_off;
    const uint2* sp_ent;
    const float* qmag;
    // hnsw_search_kernel<.., PERQ = true, QK = 3> (a batch of the coalescer that carries sparse calls, docs/hnsw.md §14): the kind
    // of every query (0, 1 or 2 as above; sp_off / sp_ent / qmag as above, a query of kind 0 or 2 owning no entries) and the
    // candidate limit it has in a launch of its own, computed by the host (a kind-1 query alone sizes its query region by its
    // entries, not by the dimension).
    const uint32_t* qkind;
    const uint32_t* qccap;
    // hnsw_search_kernel<.., MIX = true> (a handle with EmbeddingStorage::Sparse nodes, docs/hnsw.md §15): a record per node —
    // {entry offset low, high, nnz (kNone: a Dense node), bits of SparseVector::magnitude()} — and the (position, value bits) pairs
    // of all sparse nodes.  qkind / qccap are nullable there: null means kind_u for every query and the launch's own candidate limit.
    const uint4* nrec;
    const uint2* nent;
    uint32_t kind_u;
};

// Entries of the candidate heap the first launch gives a query walking with `ef` (fixed: nmn_hnsw_set_heap_capacity, 0 = default).
// No answer depends on it: a query that fills the heap is answered from scratch by the spill launch.
__host__ __device__ inline uint32_t cand_cap(uint32_t ef, uint32_t fixed, uint32_t dim, uint32_t n) {
    uint32_t c = 16u * (ef < 4096u ? ef : 4096u);
    c = c < 1024u ? 1024u : c;
    c = c > kLdsCandMax ? kLdsCandMax : c;
    if (fixed) c = fixed;
    if (dim > 4096u && c > 2048u) c = 2048u;  // (64 KiB of LDS: a long query leaves less for the heap)
    const uint32_t n1 = n ? n : 1u;
    return c < n1 ? c : n1;                   // (never more than the proven bound)
}

__device__ __forceinline__ float d_sqrt(float a) { return __builtin_sqrtf(a); }

// Distance between row `row` and the query, computed by a PAIR of lanes: lane h (0 / 1) of the pair owns the accumulator chains
// 4h .. 4h+3 and reads elements 8c + 4h .. 8c + 4h + 3 of every chunk c with one 16-byte load; the chains are the reference's eight
// (the order inside a chain is untouched), summed left to right by both lanes.  Chunks past the end read as zeros: a product +0.0
// added to a chain that is never -0.0 (it starts at +0.0) changes nothing.  Both lanes return the distance.
__device__ __forceinline__ float pair_distance(const float* __restrict__ row, float rowmag, const float* q, float qmag, uint32_t dim,
                                               int metric, uint32_t h) {
    const uint32_t chunks = dim >> 3;
    float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f, a3 = 0.0f;
    const float4* r4 = reinterpret_cast<const float4*>(row + 4u * h);
    const float4* q4 = reinterpret_cast<const float4*>(q + 4u * h);
    const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
    constexpr int PF = 4;
    const bool eu = metric == NMN_METRIC_EUCLIDEAN;
    for (uint32_t c0 = 0; c0 < chunks; c0 += PF) {
        float4 x[PF], y[PF];
#pragma unroll
        for (int i = 0; i < PF; i++) {
            const bool in = c0 + (uint32_t)i < chunks;
            x[i] = in ? r4[2u * (c0 + i)] : z;
            y[i] = in ? q4[2u * (c0 + i)] : z;
        }
#pragma unroll
        for (int i = 0; i < PF; i++) {
            if (eu) {
                const float d0 = x[i].x - y[i].x, d1 = x[i].y - y[i].y, d2 = x[i].z - y[i].z, d3 = x[i].w - y[i].w;
                a0 = a0 + d0 * d0;
                a1 = a1 + d1 * d1;
                a2 = a2 + d2 * d2;
                a3 = a3 + d3 * d3;
            } else {
                a0 = a0 + x[i].x * y[i].x;
                a1 = a1 + x[i].y * y[i].y;
                a2 = a2 + x[i].z * y[i].z;
                a3 = a3 + x[i].w * y[i].w;
            }
        }
    }
    const float b0 = __shfl_xor(a0, 1), b1 = __shfl_xor(a1, 1), b2 = __shfl_xor(a2, 1), b3 = __shfl_xor(a3, 1);
    float r = -0.0f;
    r = r + (h ? b0 : a0);
    r = r + (h ? b1 : a1);
    r = r + (h ? b2 : a2);
    r = r + (h ? b3 : a3);
    r = r + (h ? a0 : b0);
    r = r + (h ? a1 : b1);
    r = r + (h ? a2 : b2);
    r = r + (h ? a3 : b3);
    for (uint32_t i = chunks * 8u; i < dim; i++) {
        if (eu) {
            const float d = row[i] - q[i];
            r = r + d * d;
        } else {
            r = r + row[i] * q[i];
        }
    }
    if (eu) return d_sqrt(r);
    if (metric == NMN_METRIC_DOT_PRODUCT) return -r;
    if (rowmag == 0.0f || qmag == 0.0f) return 1.0f;
    return 1.0f - r / (rowmag * qmag);
}

// sum_y of dot_dense (hnsw.rs:424, 443, 450, 458): the eight chains of the query alone, by the same pair of lanes.
__device__ __forceinline__ float pair_sum(const float* q, uint32_t dim, uint32_t h) {
    const uint32_t chunks = dim >> 3;
    float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f, a3 = 0.0f;
    const float4* q4 = reinterpret_cast<const float4*>(q + 4u * h);
    for (uint32_t c = 0; c < chunks; c++) {
        const float4 y = q4[2u * c];
        a0 = a0 + y.x;
        a1 = a1 + y.y;
        a2 = a2 + y.z;
        a3 = a3 + y.w;
    }
    const float b0 = __shfl_xor(a0, 1), b1 = __shfl_xor(a1, 1), b2 = __shfl_xor(a2, 1), b3 = __shfl_xor(a3, 1);
    float r = -0.0f;
    r = r + (h ? b0 : a0);
    r = r + (h ? b1 : a1);
    r = r + (h ? b2 : a2);
    r = r + (h ? b3 : a3);
    r = r + (h ? a0 : b0);
    r = r + (h ? a1 : b1);
    r = r + (h ? a2 : b2);
    r = r + (h ? a3 : b3);
    for (uint32_t i = chunks * 8u; i < dim; i++) r = r + q[i];
    return r;
}

// distance_sparse on a Dense row under Cosine / DotProduct (hnsw.rs:1069-1079, 1143-1145): SparseVector::dot_dense
// (sparse_vector.rs:450-466) is ONE f64 chain over the query's stored entries in their order, from -0.0, each product exact in f64,
// each addition rounded once, one cast to f32.  The same PAIR of lanes as pair_distance: lane h gathers row[pos] for the entries
// 2t + h (the entries come from LDS, every pair reads the same two addresses; four gathers in flight per lane), forms its product,
// and both lanes run the chain: even entry, then odd entry, the partner's product by lane exchange.  A slot past the last entry
// contributes -0.0, which changes no sum (x + -0.0 == x for every x, -0.0 included).  Both lanes return the distance.
__device__ __forceinline__ float sparse_distance(const float* __restrict__ row, float rowmag, const uint2* ent, uint32_t nnz, float qmag,
                                                 int metric, uint32_t h) {
    double acc = -0.0;
    constexpr int PF = 4;
    for (uint32_t t0 = 0; 2u * t0 < nnz; t0 += PF) {
        uint2 e[PF];
        float x[PF];
        double pr[PF];
#pragma unroll
        for (int i = 0; i < PF; i++) {
            const uint32_t idx = 2u * (t0 + (uint32_t)i) + h;
            e[i] = idx < nnz ? ent[idx] : make_uint2(0u, 0u);
        }
#pragma unroll
        for (int i = 0; i < PF; i++) x[i] = 2u * (t0 + (uint32_t)i) + h < nnz ? row[e[i].x] : 0.0f;
#pragma unroll
        for (int i = 0; i < PF; i++)
            pr[i] = 2u * (t0 + (uint32_t)i) + h < nnz ? (double)__uint_as_float(e[i].y) * (double)x[i] : -0.0;
#pragma unroll
        for (int i = 0; i < PF; i++) {
            const double other = __shfl_xor(pr[i], 1);
            acc = acc + (h ? other : pr[i]);
            acc = acc + (h ? pr[i] : other);
        }
    }
    const float dot = (float)acc;
    if (metric == NMN_METRIC_DOT_PRODUCT) return -dot;
    if (rowmag == 0.0f || qmag == 0.0f) return 1.0f;
    return 1.0f - dot / (rowmag * qmag);
}

// distance_dense on a Sparse NODE under Cosine / DotProduct (hnsw.rs:1035-1045, 1136-1138): s.dot_dense(q), the same ONE f64
// chain from -0.0, now over the NODE's stored entries — they come from HBM with 8-byte loads, q[pos] is gathered from the query in
// LDS.  The lane mapping is sparse_distance's: lane h of the pair takes the entries 2t + h, four in flight, both lanes run the
// chain in entry order.  nmag is s.magnitude() (through f64, from the node's record), qmag the query's.
__device__ __forceinline__ float mix_dense_query(const uint2* __restrict__ ne, uint32_t nnz, float nmag, const float* q, float qmag,
                                                 int metric, uint32_t h) {
    double acc = -0.0;
    constexpr int PF = 4;
    for (uint32_t t0 = 0; 2u * t0 < nnz; t0 += PF) {
        uint2 e[PF];
        float x[PF];
        double pr[PF];
#pragma unroll
        for (int i = 0; i < PF; i++) {
            const uint32_t idx = 2u * (t0 + (uint32_t)i) + h;
            e[i] = idx < nnz ? ne[idx] : make_uint2(0u, 0u);
        }
#pragma unroll
        for (int i = 0; i < PF; i++) x[i] = 2u * (t0 + (uint32_t)i) + h < nnz ? q[e[i].x] : 0.0f;
#pragma unroll
        for (int i = 0; i < PF; i++)
            pr[i] = 2u * (t0 + (uint32_t)i) + h < nnz ? (double)__uint_as_float(e[i].y) * (double)x[i] : -0.0;
#pragma unroll
        for (int i = 0; i < PF; i++) {
            const double other = __shfl_xor(pr[i], 1);
            acc = acc + (h ? other : pr[i]);
            acc = acc + (h ? pr[i] : other);
        }
    }
    const float dot = (float)acc;
    if (metric == NMN_METRIC_DOT_PRODUCT) return -dot;
    if (nmag == 0.0f || qmag == 0.0f) return 1.0f;
    return 1.0f - dot / (nmag * qmag);
}

// distance_sparse on a Sparse NODE under Cosine / DotProduct (hnsw.rs:1069-1079, 1143-1145): s.dot(Q) is dot_f64
// (sparse_vector.rs:419-443), a two-pointer merge whose f64 accumulator starts at +0.0.  When neither side holds a duplicated
// position (the host routes every other case to its own walk) the merge is a lookup: for every node entry in order, the query entry
// of the same position, found by binary search over the sorted entries in the query region of LDS.  A miss (and a slot past the
// last entry) contributes +0.0 to a chain that starts at +0.0 and never becomes -0.0 (a product of two stored values is never a
// zero in f64, and x + (-x) rounds to +0.0), so it changes nothing.  The same pair of lanes, the same order.
__device__ __forceinline__ float mix_sparse_query(const uint2* __restrict__ ne, uint32_t nnz, float nmag, const uint2* qe, uint32_t qn,
                                                  float qmag, int metric, uint32_t h) {
    double acc = 0.0;
    constexpr int PF = 4;
    for (uint32_t t0 = 0; 2u * t0 < nnz; t0 += PF) {
        uint2 e[PF];
        double pr[PF];
#pragma unroll
        for (int i = 0; i < PF; i++) {
            const uint32_t idx = 2u * (t0 + (uint32_t)i) + h;
            e[i] = idx < nnz ? ne[idx] : make_uint2(0u, 0u);
        }
#pragma unroll
        for (int i = 0; i < PF; i++) {
            pr[i] = 0.0;
            if (2u * (t0 + (uint32_t)i) + h < nnz) {
                uint32_t lo = 0, hi = qn;
                while (lo < hi) {
                    const uint32_t mid = (lo + hi) >> 1;
                    if (qe[mid].x < e[i].x)
                        lo = mid + 1;
                    else
                        hi = mid;
                }
                if (lo < qn) {
                    const uint2 qv = qe[lo];
                    if (qv.x == e[i].x) pr[i] = (double)__uint_as_float(e[i].y) * (double)__uint_as_float(qv.y);
                }
            }
        }
#pragma unroll
        for (int i = 0; i < PF; i++) {
            const double other = __shfl_xor(pr[i], 1);
            acc = acc + (h ? other : pr[i]);
            acc = acc + (h ? pr[i] : other);
        }
    }
    const float dot = (float)acc;
    if (metric == NMN_METRIC_DOT_PRODUCT) return -dot;
    if (nmag == 0.0f || qmag == 0.0f) return 1.0f;
    return 1.0f - dot / (nmag * qmag);
}

// what a wave computes once per query: simd::magnitude (Cosine), and for quantized rows sum_y and sum_of_squares (Euclidean)
struct QuerySide {
    float mag, sum, sq;
};

__device__ __forceinline__ float ub0(uint32_t w) { return (float)(w & 0xFFu); }          // v_cvt_f32_ubyte0 .. 3
__device__ __forceinline__ float ub1(uint32_t w) { return (float)((w >> 8) & 0xFFu); }
__device__ __forceinline__ float ub2(uint32_t w) { return (float)((w >> 16) & 0xFFu); }
__device__ __forceinline__ float ub3(uint32_t w) { return (float)(w >> 24); }

// distance_dense on a ScalarQuantizedVector row, by the same PAIR of lanes as pair_distance: one 16-byte load holds the chunks 2j
// and 2j + 1; both lanes of the pair issue it (one address, one request) and lane h takes the dwords h and 2 + h of it — the codes
// 8c + 4h .. 8c + 4h + 3 of either chunk, its four chains.  A chain still sees the chunks in ascending order.  A chunk past the
// last whole one (the second half of the last load when the count is odd, where the row's tail codes or its zero padding sit, and
// the loads past the end) meets a query masked to +0.0: a code is never negative, so the product is +0.0 and changes no chain.
// The scalar tail follows the lane sum; then dot_dense's one fused multiply-add and the metric's closing arithmetic on the record.
__device__ __forceinline__ float q8_distance(const uint8_t* __restrict__ row, const float4 rec, const float* q, const QuerySide qs,
                                             uint32_t dim, int metric, uint32_t h) {
    const uint32_t chunks = dim >> 3;
    const uint32_t loads = (chunks + 1u) >> 1;
    float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f, a3 = 0.0f;
    const uint4* r16 = reinterpret_cast<const uint4*>(row);
    const float4* q4 = reinterpret_cast<const float4*>(q + 4u * h);
    const uint4 zu = make_uint4(0u, 0u, 0u, 0u);
    const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
    constexpr int PF = 4;
    for (uint32_t j0 = 0; j0 < loads; j0 += PF) {
        uint4 x[PF];
        float4 y0[PF], y1[PF];
#pragma unroll
        for (int i = 0; i < PF; i++) {
            const uint32_t j = j0 + (uint32_t)i;
            x[i] = j < loads ? r16[j] : zu;
            y0[i] = 2u * j < chunks ? q4[4u * j] : z;
            y1[i] = 2u * j + 1u < chunks ? q4[4u * j + 2u] : z;
        }
#pragma unroll
        for (int i = 0; i < PF; i++) {
            const uint32_t w0 = h ? x[i].y : x[i].x, w1 = h ? x[i].w : x[i].z;
            a0 = a0 + ub0(w0) * y0[i].x;
            a1 = a1 + ub1(w0) * y0[i].y;
            a2 = a2 + ub2(w0) * y0[i].z;
            a3 = a3 + ub3(w0) * y0[i].w;
            a0 = a0 + ub0(w1) * y1[i].x;
            a1 = a1 + ub1(w1) * y1[i].y;
            a2 = a2 + ub2(w1) * y1[i].z;
            a3 = a3 + ub3(w1) * y1[i].w;
        }
    }
    const float b0 = __shfl_xor(a0, 1), b1 = __shfl_xor(a1, 1), b2 = __shfl_xor(a2, 1), b3 = __shfl_xor(a3, 1);
    float r = -0.0f;
    r = r + (h ? b0 : a0);
    r = r + (h ? b1 : a1);
    r = r + (h ? b2 : a2);
    r = r + (h ? b3 : a3);
    r = r + (h ? a0 : b0);
    r = r + (h ? a1 : b1);
    r = r + (h ? a2 : b2);
    r = r + (h ? a3 : b3);
    for (uint32_t i = chunks * 8u; i < dim; i++) r = r + (float)row[i] * q[i];
    const float dot = __builtin_fmaf(rec.x, r, rec.y * qs.sum);  // scale.mul_add(q_dot_y, min * sum_y)
    if (metric == NMN_METRIC_DOT_PRODUCT) return -dot;
    if (metric == NMN_METRIC_EUCLIDEAN) {
        const float t = __builtin_fmaf(2.0f, -dot, rec.w + qs.sq);
        return d_sqrt(t > 0.0f ? t : 0.0f);
    }
    if (rec.z == 0.0f || qs.mag == 0.0f) return 1.0f;
    return 1.0f - dot / (rec.z * qs.mag);
}

// One whole chunk of a Binary row for a lane's four chains: `nb` holds the INVERTED bits of elements 8c + 4h .. 8c + 4h + 3 at
// bit positions s .. s + 3, y the query's four elements.  Dot: (+-1.0) * q is q with its sign kept or flipped, exactly — the sign
// bit is flipped where the row's bit is clear, no multiply.  Euclidean: d = (+-1.0) - q, then d * d rounded and added, unfused.
template <bool EU>
__device__ __forceinline__ void bin_chunk(float& a0, float& a1, float& a2, float& a3, uint32_t nb, uint32_t s, const float4 y) {
    const uint32_t f0 = (nb << (31u - s)) & 0x80000000u, f1 = (nb << (30u - s)) & 0x80000000u;
    const uint32_t f2 = (nb << (29u - s)) & 0x80000000u, f3 = (nb << (28u - s)) & 0x80000000u;
    if (EU) {
        const float d0 = __uint_as_float(0x3F800000u | f0) - y.x, d1 = __uint_as_float(0x3F800000u | f1) - y.y;
        const float d2 = __uint_as_float(0x3F800000u | f2) - y.z, d3 = __uint_as_float(0x3F800000u | f3) - y.w;
        a0 = a0 + d0 * d0;
        a1 = a1 + d1 * d1;
        a2 = a2 + d2 * d2;
        a3 = a3 + d3 * d3;
    } else {
        a0 = a0 + __uint_as_float(__float_as_uint(y.x) ^ f0);
        a1 = a1 + __uint_as_float(__float_as_uint(y.y) ^ f1);
        a2 = a2 + __uint_as_float(__float_as_uint(y.z) ^ f2);
        a3 = a3 + __uint_as_float(__float_as_uint(y.w) ^ f3);
    }
}

// One 16-byte load of a Binary row: chunks 0 .. lim - 1 of its sixteen (FULL: all of them, no test), a dword — four chunks — per
// turn of a loop that is NOT unrolled, to keep the code short: the dword is picked by wave-uniform selects.
template <bool EU, bool FULL>
__device__ __forceinline__ void bin_load16(float& a0, float& a1, float& a2, float& a3, const uint4 x, uint32_t lim, uint32_t sh,
                                           const float4* qj) {
#pragma unroll 1
    for (uint32_t d = 0; d < 4u; d++) {
        if (!FULL && 4u * d >= lim) break;
        const uint32_t nb = ~(d == 0u ? x.x : (d == 1u ? x.y : (d == 2u ? x.z : x.w)));
        const float4* qd = qj + 8u * d;
#pragma unroll
        for (uint32_t b = 0; b < 4u; b++)
            if (FULL || 4u * d + b < lim) bin_chunk<EU>(a0, a1, a2, a3, nb, 8u * b + sh, qd[2u * b]);
    }
}

// distance_dense on a BinaryVector row, by the same PAIR of lanes as pair_distance.  One 16-byte load carries 128 bits, sixteen
// chunks of eight; both lanes of the pair issue it (one address, one request) and lane h takes bits 8c + 4h .. 8c + 4h + 3 of every
// chunk c, its four chains, in ascending c.  `full` loads hold sixteen whole chunks each and run PF at a time without a test per
// chunk; the one load after them (when dim is no multiple of 128) holds the remaining whole chunks and the tail bits, is issued
// before the others, and is walked under the test `chunk < rem` — dim is wave-uniform, so the test is a scalar branch and a chunk
// past the last whole one contributes NOTHING: no term is formed for it (what masking the query to +0.0 would give the dot, and what
// Euclidean needs, where (-1 - 0)^2 = 1).  A 128-dimension row is the single load of the first pass.  The scalar tail follows the
// lane sum, bit by bit.  Both lanes return the sum.
template <bool EU>
__device__ __forceinline__ float bin_sum(const uint8_t* __restrict__ row, const float* q, uint32_t dim, uint32_t h) {
    const uint32_t chunks = dim >> 3, full = chunks >> 4, rem = chunks & 15u;
    float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f, a3 = 0.0f;
    const uint4* r16 = reinterpret_cast<const uint4*>(row);
    const float4* q4 = reinterpret_cast<const float4*>(q + 4u * h);
    const uint4 zu = make_uint4(0u, 0u, 0u, 0u);
    const uint32_t sh = 4u * h;
    uint4 xr = zu;
    if ((dim & 127u) != 0u) xr = r16[full];  // (the row's last 16 bytes: ld8 = 16 ceil(dim / 128))
    constexpr int PF = 4;
    for (uint32_t j0 = 0; j0 < full; j0 += PF) {
        uint4 x[PF];
#pragma unroll
        for (int i = 0; i < PF; i++) x[i] = j0 + (uint32_t)i < full ? r16[j0 + (uint32_t)i] : zu;
#pragma unroll
        for (int i = 0; i < PF; i++) {
            const uint32_t j = j0 + (uint32_t)i;
            if (j < full) bin_load16<EU, true>(a0, a1, a2, a3, x[i], 16u, sh, q4 + 32u * j);
        }
    }
    if (rem) bin_load16<EU, false>(a0, a1, a2, a3, xr, rem, sh, q4 + 32u * full);
    const float b0 = __shfl_xor(a0, 1), b1 = __shfl_xor(a1, 1), b2 = __shfl_xor(a2, 1), b3 = __shfl_xor(a3, 1);
    float r = -0.0f;
    r = r + (h ? b0 : a0);
    r = r + (h ? b1 : a1);
    r = r + (h ? b2 : a2);
    r = r + (h ? b3 : a3);
    r = r + (h ? a0 : b0);
    r = r + (h ? a1 : b1);
    r = r + (h ? a2 : b2);
    r = r + (h ? a3 : b3);
    const uint32_t tail = dim & 7u;
    if (tail) {  // byte `rem` of the last load: the bits of elements 8 chunks .. dim - 1
        const uint32_t dw = rem >> 2;
        const uint32_t wv = dw == 0u ? xr.x : (dw == 1u ? xr.y : (dw == 2u ? xr.z : xr.w));
        const uint32_t tb = wv >> (8u * (rem & 3u));
        for (uint32_t t = 0; t < tail; t++) {
            const float e = ((tb >> t) & 1u) ? 1.0f : -1.0f;
            const float y = q[8u * chunks + t];
            if (EU) {
                const float d = e - y;
                r = r + d * d;
            } else {
                r = r + (e > 0.0f ? y : -y);
            }
        }
    }
    return r;
}
__device__ __forceinline__ float bin_distance(const uint8_t* __restrict__ row, const float* q, float qmag, float sqrt_dim, uint32_t dim,
                                              int metric, uint32_t h) {
    if (metric == NMN_METRIC_EUCLIDEAN) return d_sqrt(bin_sum<true>(row, q, dim, h));
    const float r = bin_sum<false>(row, q, dim, h);
    if (metric == NMN_METRIC_DOT_PRODUCT) return -r;
    if (qmag == 0.0f) return 1.0f;
    return 1.0f - r / (sqrt_dim * qmag);
}

// One query per wave (one wave per workgroup).  SPILL == false: both heaps in LDS; a query whose candidate heap fills up is flagged
// and left.  SPILL == true: workgroup b answers the flagged queries b, b + grid, ... from scratch with both heaps in its region of
// global memory (candidates: n entries, the proven bound — nothing is pushed twice).
// Only lane 0 touches the heaps; the other lanes learn what to do next through `ctrl` in LDS.
// Q8 == true: the rows are ScalarQuantizedVectors (codes + a record per row), scored by q8_distance.
// PERQ == true: k and ef are the query's own (a.qk / a.qef, read once per query: a wave serves one query, so they are
// wave-uniform), rows of the outputs are a.kstride apart.  PERQ == false is the kernel as it has always been.
// QK: the query kind.  0: a dense query, everything above.  1 (dense rows, Cosine / DotProduct): the query is a SparseVector — its
// stored entries sit in the query region of LDS as (u32 position, f32 value) pairs, rows are scored by sparse_distance, and the
// query's magnitude is a.qmag[q].  2 (quantized rows): a dense query whose Cosine magnitude is a.qmag[q] instead of the
// simd::magnitude the wave computes.  3 (PERQ only): the kind is the query's own, a.qkind[q] — 0 or 1 on dense rows, 0 or 2 on
// quantized rows — and so is its candidate limit, a.qccap[q]; a wave serves one query, so every branch on the kind is
// wave-uniform.  QK is a template parameter so that the QK == 0 instantiations stay the code they were.
// MIX (dense rows, PERQ, QK == 3; Cosine / DotProduct): the handle holds EmbeddingStorage::Sparse nodes.  row_distance reads the
// node's record and scores a sparse node from its stored entries (mix_dense_query / mix_sparse_query); a Dense node keeps the
// arithmetic above.  The two lanes of a pair score one node and agree on its kind; the pairs of one pass may not, so both sides run
// under exec masks — the one lane-divergent branch of the scoring path.  These instantiations serve uniform launches as well
// (a.qk / a.qef / a.qkind / a.qccap null).  MIX is a template parameter so that every other instantiation stays the code it was.
// BIN (dense queries only: QK == 0): the rows are BinaryVectors — g.codes holds their words, g.ld8 apart — scored by bin_distance;
// nothing else of the walk changes.  BIN is a template parameter for the same reason.
template <bool SPILL, bool Q8, bool PERQ, int QK = 0, bool MIX = false, bool BIN = false>
__global__ __launch_bounds__(64) void hnsw_search_kernel(SearchArgs a) {
    static_assert(QK == 0 || (QK == 1 && !Q8 && !PERQ) || (QK == 2 && Q8 && !PERQ) || (QK == 3 && PERQ),
                  "query kinds: 1 on dense rows, 2 on quantized rows, 3 = a kind per query of a per-query launch");
    static_assert(!MIX || (!Q8 && PERQ && QK == 3), "sparse nodes: dense storage, the per-query form");
    static_assert(!BIN || (!Q8 && QK == 0 && !MIX), "binary rows: dense queries, a storage of their own");
    extern __shared__ float4 smem4[];
    const GraphDev& g = a.g;
    const uint32_t lane = threadIdx.x, p = lane >> 1, h = lane & 1u;
    float* qs = reinterpret_cast<float*>(smem4);
    uint32_t* stage_id = reinterpret_cast<uint32_t*>(qs + a.qlds);
    float* stage_d = reinterpret_cast<float*>(stage_id + 32);
    uint32_t* ctrl = reinterpret_cast<uint32_t*>(stage_d + 32);  // [0] done, [1] current node, [2] overflow, [3] results
    Ent* R;
    Ent* Cn;
    if (SPILL) {
        R = a.spill + (size_t)blockIdx.x * ((size_t)a.rcap + a.ccap);
        Cn = R + a.rcap;
    } else {
        R = reinterpret_cast<Ent*>(ctrl + 4);
        Cn = R + a.rcap;
    }
    const float ninf = __int_as_float(0xFF800000u);
    for (uint32_t q = blockIdx.x; q < a.nq; q += gridDim.x) {
        if (SPILL && a.flags[q] != 1u) continue;
        const float* qg = a.queries + (size_t)q * g.dim;
        const float* qv = qs;
        __syncthreads();
        uint32_t nnz = 0;
        bool entries = QK == 1;             // the query region holds stored entries, rows are scored by sparse_distance
        bool mag_given = QK == 1 || QK == 2;  // the Cosine magnitude is a.qmag[q]
        if constexpr (QK == 3) {
            const uint32_t kind = MIX && !a.qkind ? a.kind_u : a.qkind[q];
            entries = !Q8 && kind == 1u;
            mag_given = kind != 0u;
        }
        if (QK != 0 && QK != 2 && entries) {
            const uint64_t e0 = a.sp_off[q];
            nnz = min((uint32_t)(a.sp_off[q + 1] - e0), a.qlds >> 1);  // (the host sized the region by the launch's largest count)
            uint2* el = reinterpret_cast<uint2*>(qs);
            for (uint32_t i = lane; i < nnz; i += 64) el[i] = a.sp_ent[e0 + i];
        } else {
            for (uint32_t i = lane; i < a.qlds; i += 64) qs[i] = i < g.dim ? qg[i] : 0.0f;
        }
        uint32_t* vis = a.visited + (size_t)q * a.vwords;
        if (SPILL) {
            for (uint32_t w = lane; w < a.vwords; w += 64) vis[w] = 0u;
            __threadfence();
        }
        __syncthreads();
        const uint32_t k_q = PERQ && a.qk ? a.qk[q] : a.k;
        const uint32_t ef_q = PERQ && a.qef ? a.qef[q] : a.ef;
        const uint32_t kstride = PERQ ? a.kstride : a.k;
        const uint32_t ccap_q =
            PERQ && !SPILL ? min(a.ccap, QK == 3 ? (MIX && !a.qccap ? a.ccap : a.qccap[q]) : cand_cap(ef_q, a.ccap_fixed, g.dim, g.n))
                           : a.ccap;
        uint64_t* o_ids = a.out_ids + (size_t)q * kstride;
        float* o_sc = a.out_scores + (size_t)q * kstride;
        if (g.n == 0 || g.entry == kNone) {  // hnsw.rs:2070-2073
            for (uint32_t i = lane; i < kstride; i += 64) {
                o_ids[i] = ~0ull;
                o_sc[i] = ninf;
            }
            if (lane == 0) {
                a.out_counts[q] = 0;
                a.evals[q] = 0;
                if (SPILL) a.flags[q] = 2u;
            }
            continue;
        }
        float qmag = 0.0f;
        if (QK == 0 || !mag_given) {
            if (g.metric == NMN_METRIC_COSINE) qmag = d_sqrt(-pair_distance(qv, 0.f, qv, 0.f, g.dim, NMN_METRIC_DOT_PRODUCT, h));
        } else {
            if (g.metric == NMN_METRIC_COSINE) qmag = a.qmag[q];
        }
        QuerySide qside{qmag, 0.0f, 0.0f};
        if (Q8) {
            qside.sum = pair_sum(qv, g.dim, h);
            if (g.metric == NMN_METRIC_EUCLIDEAN) qside.sq = -pair_distance(qv, 0.f, qv, 0.f, g.dim, NMN_METRIC_DOT_PRODUCT, h);
        }
        float sqrt_dim = 0.0f;
        if constexpr (BIN) sqrt_dim = d_sqrt((float)g.dim);  // (dimension as f32).sqrt(), hnsw.rs:981-984
        auto row_distance = [&](uint32_t node) -> float {
            if constexpr (BIN) return bin_distance(g.codes + (size_t)node * g.ld8, qv, qmag, sqrt_dim, g.dim, g.metric, h);
            if constexpr (MIX) {
                const uint4 rec = a.nrec[node];
                if (rec.z != kNone) {
                    const uint2* ne = a.nent + (((uint64_t)rec.y << 32) | rec.x);
                    const float nmag = __uint_as_float(rec.w);
                    if (entries) return mix_sparse_query(ne, rec.z, nmag, reinterpret_cast<const uint2*>(qv), nnz, qmag, g.metric, h);
                    return mix_dense_query(ne, rec.z, nmag, qv, qmag, g.metric, h);
                }
            }
            if (QK != 0 && QK != 2 && entries)
                return sparse_distance(g.corpus + (size_t)node * g.ld, g.norms[node], reinterpret_cast<const uint2*>(qv), nnz, qmag,
                                       g.metric, h);
            else if constexpr (Q8)
                return q8_distance(g.codes + (size_t)node * g.ld8, g.rec[node], qv, qside, g.dim, g.metric, h);
            else
                return pair_distance(g.corpus + (size_t)node * g.ld, g.norms[node], qv, qmag, g.dim, g.metric, h);
        };
        // distance evaluations.  The reference scores the entry of every search_layer* call again (one per greedy layer, one for
        // search_layer); this kernel carries the distance along.  A quantized or binary handle counts the evaluations the reference makes,
        // as the host walk does; a dense handle keeps the count it has always reported.
        uint32_t evals = Q8 || BIN ? g.max_layer + 1u : 1u;
        // greedy descent, hnsw.rs:2086-2092 / 2170-2200
        uint32_t cur = g.entry;
        float cur_d = row_distance(cur);
        for (uint32_t layer = g.max_layer; layer >= 1; layer--) {
            for (;;) {
                const uint32_t ui = g.up_idx[cur];
                const size_t slot = (size_t)ui * g.up_layers + (layer - 1);
                const uint32_t cnt = ui == kNone ? 0u : g.upcnt[slot];
                const uint32_t* base = g.up + slot * g.m;
                uint32_t best = cur;
                float best_d = cur_d;
                for (uint32_t j0 = 0; j0 < cnt; j0 += 32) {
                    const uint32_t j = j0 + p;
                    uint32_t nid = kNone;
                    float d = 0.0f;
                    if (j < cnt) {
                        nid = base[j];
                        d = row_distance(nid);
                    }
                    __syncthreads();
                    if (h == 0) {
                        stage_id[p] = nid;
                        stage_d[p] = d;
                    }
                    __syncthreads();
                    const uint32_t lim = min(32u, cnt - j0);
                    for (uint32_t t = 0; t < lim; t++) {  // every lane, the same reads: the list in id order
                        const float dt = stage_d[t];
                        if (dt < best_d) {
                            best = stage_id[t];
                            best_d = dt;
                        }
                    }
                }
                evals += cnt;
                if (best == cur) break;  // (`changed` is false exactly when no neighbour was strictly closer)
                cur = best;
                cur_d = best_d;
            }
        }
        // layer 0: search_layer, hnsw.rs:2276-2335
        uint32_t rn = 0, cn = 0;  // (lane 0's are the real ones)
        if (lane == 0) {
            atomicOr(&vis[cur >> 5], 1u << (cur & 31u));
            heap_push<false>(Cn, cn, Ent{cur_d, cur});
            heap_push<true>(R, rn, Ent{cur_d, cur});
            ctrl[2] = 0;
        }
        bool overflow = false;
        for (;;) {
            __syncthreads();
            if (lane == 0) {
                uint32_t done = 0, c = 0;
                if (cn == 0) {
                    done = 1;
                } else {
                    const Ent e = heap_pop<false>(Cn, cn);
                    c = e.id;
                    if (rn >= ef_q && e.d > R[0].d) done = 1;
                }
                ctrl[0] = done;
                ctrl[1] = c;
            }
            __syncthreads();
            if (ctrl[0]) break;
            const uint32_t c = ctrl[1];
            const uint32_t cnt = g.l0cnt[c];
            const uint32_t* base = g.l0 + (size_t)c * g.m0;
            for (uint32_t j0 = 0; j0 < cnt; j0 += 32) {
                const uint32_t j = j0 + p;
                uint32_t nid = kNone;
                float d = 0.0f;
                if (j < cnt) {
                    nid = base[j];
                    uint32_t seen = 0;
                    if (h == 0) seen = (atomicOr(&vis[nid >> 5], 1u << (nid & 31u)) >> (nid & 31u)) & 1u;
                    seen = __shfl(seen, (int)(lane & ~1u));
                    if (seen)
                        nid = kNone;
                    else
                        d = row_distance(nid);
                }
                if (h == 0) {
                    stage_id[p] = nid;
                    stage_d[p] = d;
                }
                __syncthreads();
                if (lane == 0) {
                    const uint32_t lim = min(32u, cnt - j0);
                    for (uint32_t t = 0; t < lim; t++) {
                        const uint32_t id = stage_id[t];
                        if (id == kNone) continue;
                        evals++;
                        const float dt = stage_d[t];
                        const bool should_add = rn < ef_q || dt < R[0].d;
                        if (should_add) {
                            if (cn == ccap_q) {
                                ctrl[2] = 1;
                                break;
                            }
                            heap_push<false>(Cn, cn, Ent{dt, id});
                            heap_push<true>(R, rn, Ent{dt, id});
                            while (rn > ef_q) (void)heap_pop<true>(R, rn);
                        }
                    }
                }
                __syncthreads();
                if (ctrl[2]) {
                    overflow = true;
                    break;
                }
            }
            if (overflow) break;
        }
        if (overflow) {  // the spill launch answers this query; nothing of it has been written
            if (lane == 0) a.flags[q] = 1u;
            continue;
        }
        if (lane == 0) ctrl[3] = rn;
        if (SPILL) __threadfence();
        __syncthreads();
        const uint32_t n_res = ctrl[3];
        const uint32_t count = min(k_q, n_res);
        // stable sort by distance of the vector order (hnsw.rs:2328-2333), as ranks: element e goes to
        // #{j : d_j < d_e} + #{j < e : d_j == d_e}
        for (uint32_t e = lane; e < n_res; e += 64) {
            const Ent me = R[e];
            uint32_t rank = 0;
            for (uint32_t j = 0; j < n_res; j++) {
                const float dj = R[j].d;
                rank += (dj < me.d || (dj == me.d && j < e)) ? 1u : 0u;
            }
            if (rank < k_q) {
                o_ids[rank] = (uint64_t)me.id;
                o_sc[rank] = to_similarity(g.metric, me.d);
            }
        }
        for (uint32_t i = count + lane; i < kstride; i += 64) {
            o_ids[i] = ~0ull;
            o_sc[i] = ninf;
        }
        if (lane == 0) {
            a.out_counts[q] = count;
            a.evals[q] = evals;
            if (SPILL) a.flags[q] = 2u;
        }
    }
}

// ---- the build walk (nmn_hnsw_insert_bulk, docs/hnsw.md §19) ----------------------------------------------------------------------
// What try_insert_embedding (hnsw.rs:1936-2051) SEARCHES for one new node, against the graph as it sits in HBM at launch: the
// greedy descent above the node's level, then search_layer with ef_construction on every layer from min(level, max_layer) down,
// the first sorted result of a layer the entry of the next.  Nothing is committed here: the host takes the selections of a walk
// only when none of the lists it read has been assigned since the launch, so the kernel also reports which lists it read.
struct InsertArgs {
    GraphDev g;             // the snapshot: n nodes, its entry and max_layer; `up` laid out at the call's final up_layers
    const uint8_t* levels;  // the levels of the call's rows: node id has levels[id - lv_base]
    uint32_t lv_base;
    uint32_t first, nb;     // the batch: nodes first .. first + nb - 1, their rows already in g.corpus
    uint32_t ef, rcap, ccap, qlds;
    uint32_t* visited;      // [nb][vwords]
    uint32_t vwords;
    uint32_t sel_stride;    // m0 + max_layer * m: layer 0's selections first, layer l >= 1 at m0 + (l - 1) * m
    uint32_t rd_cap;
    uint32_t* status;       // [nb] 0 = walked, 1 = the candidate heap or the read list filled: the host walks this node
    uint32_t* selcnt;       // [nb][max_layer + 1] min(m or m0, found) per searched layer
    uint32_t* rdend;        // [nb][max_layer + 1] end of the layer's reads in the node's read list; the layers run max_layer .. 0
    uint32_t* sel;          // [nb][sel_stride] the first selcnt ids of search_layer's result, in its stable order
    uint32_t* reads;        // [nb][rd_cap] the nodes whose list at the layer was read: greedy's round starts, search_layer's pops
};

// One new node per wave (one wave per workgroup), the walk of hnsw_search_kernel<false, false, false> with three changes: the
// query is the node's own row, search_layer runs on the upper layers too (their lists through up_idx), and a fresh visited set and
// empty heaps per layer.  Only lane 0 touches the heaps and the read list.
__global__ __launch_bounds__(64) void hnsw_insert_walk_kernel(InsertArgs a) {
    extern __shared__ float4 smem4[];
    const GraphDev& g = a.g;
    const uint32_t lane = threadIdx.x, p = lane >> 1, h = lane & 1u;
    float* qs = reinterpret_cast<float*>(smem4);
    uint32_t* stage_id = reinterpret_cast<uint32_t*>(qs + a.qlds);
    float* stage_d = reinterpret_cast<float*>(stage_id + 32);
    // [0] done, [1] current node, [2] overflow, [3] results, [4] / [5] the first sorted result and its distance
    uint32_t* ctrl = reinterpret_cast<uint32_t*>(stage_d + 32);
    Ent* R = reinterpret_cast<Ent*>(ctrl + 8);
    Ent* Cn = R + a.rcap;
    const uint32_t layers = g.max_layer + 1u;
    for (uint32_t b = blockIdx.x; b < a.nb; b += gridDim.x) {
        const uint32_t id = a.first + b;
        const uint32_t lq = a.levels[id - a.lv_base];
        const float* qg = g.corpus + (size_t)id * g.ld;
        const float* qv = qs;
        __syncthreads();
        for (uint32_t i = lane; i < a.qlds; i += 64) qs[i] = i < g.dim ? qg[i] : 0.0f;
        if (lane == 0) ctrl[2] = 0;
        uint32_t* vis = a.visited + (size_t)b * a.vwords;
        uint32_t* rd = a.reads + (size_t)b * a.rd_cap;
        uint32_t* o_end = a.rdend + (size_t)b * layers;
        __syncthreads();
        float qmag = 0.0f;
        if (g.metric == NMN_METRIC_COSINE) qmag = d_sqrt(-pair_distance(qv, 0.f, qv, 0.f, g.dim, NMN_METRIC_DOT_PRODUCT, h));
        auto row_distance = [&](uint32_t node) -> float {
            return pair_distance(g.corpus + (size_t)node * g.ld, g.norms[node], qv, qmag, g.dim, g.metric, h);
        };
        uint32_t nrd = 0;  // entries of the read list (every lane counts through the descent, lane 0 alone after it)
        bool overflow = false;
        // greedy descent on the layers above the node's level, hnsw.rs:1989-1992 / 2170-2200
        uint32_t cur = g.entry;
        float cur_d = row_distance(cur);
        for (uint32_t layer = g.max_layer; layer > lq && !overflow; layer--) {
            for (;;) {
                if (nrd == a.rd_cap) {
                    overflow = true;
                    break;
                }
                if (lane == 0) rd[nrd] = cur;
                nrd++;
                const uint32_t ui = g.up_idx[cur];
                const size_t slot = (size_t)ui * g.up_layers + (layer - 1);
                const uint32_t cnt = ui == kNone ? 0u : g.upcnt[slot];
                const uint32_t* base = g.up + slot * g.m;
                uint32_t best = cur;
                float best_d = cur_d;
                for (uint32_t j0 = 0; j0 < cnt; j0 += 32) {
                    const uint32_t j = j0 + p;
                    uint32_t nid = kNone;
                    float d = 0.0f;
                    if (j < cnt) {
                        nid = base[j];
                        d = row_distance(nid);
                    }
                    __syncthreads();
                    if (h == 0) {
                        stage_id[p] = nid;
                        stage_d[p] = d;
                    }
                    __syncthreads();
                    const uint32_t lim = min(32u, cnt - j0);
                    for (uint32_t t = 0; t < lim; t++) {
                        const float dt = stage_d[t];
                        if (dt < best_d) {
                            best = stage_id[t];
                            best_d = dt;
                        }
                    }
                }
                if (best == cur) break;
                cur = best;
                cur_d = best_d;
            }
            if (lane == 0) o_end[layer] = nrd;
        }
        // search_layer with ef_construction per layer, hnsw.rs:1994-2044 / 2276-2335
        for (int layer = (int)min(lq, g.max_layer); layer >= 0 && !overflow; layer--) {
            for (uint32_t w = lane; w < a.vwords; w += 64) vis[w] = 0u;  // a fresh visited set per call
            __threadfence();
            __syncthreads();
            uint32_t rn = 0, cn = 0;  // (lane 0's are the real ones): both heaps start empty
            if (lane == 0) {
                atomicOr(&vis[cur >> 5], 1u << (cur & 31u));
                heap_push<false>(Cn, cn, Ent{cur_d, cur});
                heap_push<true>(R, rn, Ent{cur_d, cur});
            }
            for (;;) {
                __syncthreads();
                if (lane == 0) {
                    uint32_t done = 0, c = 0;
                    if (cn == 0) {
                        done = 1;
                    } else {
                        const Ent e = heap_pop<false>(Cn, cn);
                        c = e.id;
                        if (rn >= a.ef && e.d > R[0].d) {
                            done = 1;
                        } else if (nrd == a.rd_cap) {
                            ctrl[2] = 1;
                            done = 1;
                        } else {
                            rd[nrd++] = c;
                        }
                    }
                    ctrl[0] = done;
                    ctrl[1] = c;
                }
                __syncthreads();
                if (ctrl[0]) break;
                const uint32_t c = ctrl[1];
                uint32_t cnt;
                const uint32_t* base;
                if (layer == 0) {
                    cnt = g.l0cnt[c];
                    base = g.l0 + (size_t)c * g.m0;
                } else {
                    const uint32_t ui = g.up_idx[c];
                    const size_t slot = (size_t)ui * g.up_layers + (uint32_t)(layer - 1);
                    cnt = ui == kNone ? 0u : g.upcnt[slot];
                    base = g.up + slot * g.m;
                }
                for (uint32_t j0 = 0; j0 < cnt; j0 += 32) {
                    const uint32_t j = j0 + p;
                    uint32_t nid = kNone;
                    float d = 0.0f;
                    if (j < cnt) {
                        nid = base[j];
                        uint32_t seen = 0;
                        if (h == 0) seen = (atomicOr(&vis[nid >> 5], 1u << (nid & 31u)) >> (nid & 31u)) & 1u;
                        seen = __shfl(seen, (int)(lane & ~1u));
                        if (seen)
                            nid = kNone;
                        else
                            d = row_distance(nid);
                    }
                    if (h == 0) {
                        stage_id[p] = nid;
                        stage_d[p] = d;
                    }
                    __syncthreads();
                    if (lane == 0) {
                        const uint32_t lim = min(32u, cnt - j0);
                        for (uint32_t t = 0; t < lim; t++) {
                            const uint32_t nid_t = stage_id[t];
                            if (nid_t == kNone) continue;
                            const float dt = stage_d[t];
                            const bool should_add = rn < a.ef || dt < R[0].d;
                            if (should_add) {
                                if (cn == a.ccap) {
                                    ctrl[2] = 1;
                                    break;
                                }
                                heap_push<false>(Cn, cn, Ent{dt, nid_t});
                                heap_push<true>(R, rn, Ent{dt, nid_t});
                                while (rn > a.ef) (void)heap_pop<true>(R, rn);
                            }
                        }
                    }
                    __syncthreads();
                    if (ctrl[2]) break;
                }
                if (ctrl[2]) break;
            }
            if (ctrl[2]) {
                overflow = true;
                break;
            }
            if (lane == 0) ctrl[3] = rn;
            __syncthreads();
            const uint32_t n_res = ctrl[3];
            const uint32_t m_l = layer == 0 ? g.m0 : g.m;
            uint32_t* o_sel = a.sel + (size_t)b * a.sel_stride + (layer == 0 ? 0u : g.m0 + (uint32_t)(layer - 1) * g.m);
            // the stable sort by distance of the vector order as ranks (hnsw_search_kernel); only the first m_l are used
            for (uint32_t e = lane; e < n_res; e += 64) {
                const Ent me = R[e];
                uint32_t rank = 0;
                for (uint32_t j = 0; j < n_res; j++) {
                    const float dj = R[j].d;
                    rank += (dj < me.d || (dj == me.d && j < e)) ? 1u : 0u;
                }
                if (rank < m_l) o_sel[rank] = me.id;
                if (rank == 0) {  // `current_node = neighbors[0].id`, its distance carried along
                    ctrl[4] = me.id;
                    ctrl[5] = __float_as_uint(me.d);
                }
            }
            if (lane == 0) {
                a.selcnt[(size_t)b * layers + (uint32_t)layer] = min(m_l, n_res);
                o_end[layer] = nrd;
            }
            __syncthreads();
            cur = ctrl[4];
            cur_d = __uint_as_float(ctrl[5]);
        }
        if (lane == 0) a.status[b] = overflow ? 1u : 0u;
    }
}

// The lists the host's commits assigned since the last launch, scattered into the adjacency in HBM: a record of `stride` words per
// workgroup turn — {kind, slot, count, ids ...}.  kind 0: layer-0 list of node `slot`; 1: upper list at slot `slot` of up / upcnt;
// 2: up_idx[slot] = count.  The host sends every list once per batch, so no two records of a launch share a target.
struct PatchArgs {
    uint32_t* l0;
    uint32_t* l0cnt;
    uint32_t* up_idx;
    uint32_t* up;
    uint32_t* upcnt;
    const uint32_t* rec;
    uint32_t nrec, stride, m, m0;
    uint64_t nodes, up_slots;  // what the arrays were allocated for
};
__global__ __launch_bounds__(64) void hnsw_patch_kernel(PatchArgs a) {
    for (uint32_t r = blockIdx.x; r < a.nrec; r += gridDim.x) {
        const uint32_t* rec = a.rec + (size_t)r * a.stride;
        const uint32_t kind = rec[0], slot = rec[1], cnt = rec[2];
        if (kind == 0u) {
            if (slot >= a.nodes || cnt > a.m0) continue;
            for (uint32_t t = threadIdx.x; t < a.m0; t += 64) a.l0[(size_t)slot * a.m0 + t] = t < cnt ? rec[3 + t] : kNone;
            if (threadIdx.x == 0) a.l0cnt[slot] = cnt;
        } else if (kind == 1u) {
            if (slot >= a.up_slots || cnt > a.m) continue;
            for (uint32_t t = threadIdx.x; t < a.m; t += 64) a.up[(size_t)slot * a.m + t] = t < cnt ? rec[3 + t] : kNone;
            if (threadIdx.x == 0) a.upcnt[slot] = cnt;
        } else if (slot < a.nodes && threadIdx.x == 0) {
            a.up_idx[slot] = cnt;
        }
    }
}

struct DevBuf {
    void* p = nullptr;
    size_t cap = 0;
};

}  // namespace

}  // namespace nmn

using namespace nmn;

struct nmn_hnsw {
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
    std::vector<uint8_t> level;
    std::vector<std::vector<std::vector<uint32_t>>> nbr;  // [node][layer], id-ascending
    uint64_t entry = ~0ull;
    uint32_t max_layer = 0;
    uint64_t rng = 42;  // hnsw.rs:1584
    // device side
    DevBuf d_l0, d_l0cnt, d_upidx, d_up, d_upcnt;
    DevBuf d_nrec, d_nent;  // a handle with sparse nodes: the record per node and the entries of all sparse nodes (SearchArgs)
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

namespace {

#define HN_TRY(expr)                                                  \
    do {                                                              \
        hipError_t _e = (expr);                                       \
        if (_e != hipSuccess) return set_error_hip(_e, #expr);        \
    } while (0)

hipError_t grow(DevBuf& b, size_t bytes, hipStream_t s, bool* synced) {
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
void drop(DevBuf& b) {
    if (b.p) (void)hipFree(b.p);
    b.p = nullptr;
    b.cap = 0;
}

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

// the query side: distance_dense(stored row `node`, q).  A Sparse node (hnsw.rs:1035-1045, 1084-1091, 1136-1138): s.dot_dense(q)
// with s.magnitude() under Cosine / DotProduct, simd::euclidean_distance(s.to_dense(), q) — the row kept here — under Euclidean.
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
    return h_distance(metric, h->rows.data() + (size_t)b * h->dim, h->mags[b], h->rows.data() + (size_t)a * h->dim, h->mags[a],
                      h->dim);
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

void host_search_one(const nmn_hnsw* h, const float* q, uint32_t k, uint64_t ef, HostVisited& vis, uint64_t* ids, float* scores,
                     uint32_t* count, uint64_t* evals) {
    const HQ qmag = host_query(h, q);
    host_walk_one(h, [&](uint32_t node) { return node_distance(h, node, q, qmag); }, k, ef, vis, ids, scores, count, evals);
}

// ---- SparseVector queries (sparse_vector.rs:155-193, 400-406, 450-466, 548-559; docs/hnsw.md §13) --------------------------------
// dot_dense and magnitude are h_sparse_dot / h_sparse_mag above.

// The queries of one nmn_hnsw_search_sparse call as SparseVector::try_from_parts leaves them: entries with val == 0.0 (either sign)
// dropped, NaN kept, the rest stably sorted by position (duplicates survive in input order).  (Named in nmn:: because a HostWalk
// carries a pointer to it through the coalescer, nmn_hnsw_queue.h.)
}  // namespace
namespace nmn {
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
namespace {

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
nmn_status upload_graph(nmn_hnsw* h, size_t reserve_n = 0, uint32_t reserve_upper = 0, uint32_t layers = 0) {
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

SearchArgs graph_args(const nmn_hnsw* h, uint32_t n) {
    SearchArgs a{};
    a.g.corpus = h->vectors ? h->vectors->corpus : nullptr;
    a.g.norms = h->vectors ? h->vectors->norms : nullptr;
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

template <bool SPILL>
void launch_walk(bool q8, bool bin, bool perq, int qkind, bool mix, uint32_t grid, size_t lds, hipStream_t s, const SearchArgs& a) {
    if (bin && perq)  // binary rows: dense queries only (every other query form is refused before it gets here)
        hipLaunchKernelGGL((hnsw_search_kernel<SPILL, false, true, 0, false, true>), dim3(grid), dim3(64), lds, s, a);
    else if (bin)
        hipLaunchKernelGGL((hnsw_search_kernel<SPILL, false, false, 0, false, true>), dim3(grid), dim3(64), lds, s, a);
    else if (mix)  // a handle with sparse nodes, Cosine / DotProduct: one form for uniform and per-query launches alike
        hipLaunchKernelGGL((hnsw_search_kernel<SPILL, false, true, 3, true>), dim3(grid), dim3(64), lds, s, a);
    else if (qkind == 3 && q8)
        hipLaunchKernelGGL((hnsw_search_kernel<SPILL, true, true, 3>), dim3(grid), dim3(64), lds, s, a);
    else if (qkind == 3)
        hipLaunchKernelGGL((hnsw_search_kernel<SPILL, false, true, 3>), dim3(grid), dim3(64), lds, s, a);
    else if (qkind == 1)
        hipLaunchKernelGGL((hnsw_search_kernel<SPILL, false, false, 1>), dim3(grid), dim3(64), lds, s, a);
    else if (qkind == 2)
        hipLaunchKernelGGL((hnsw_search_kernel<SPILL, true, false, 2>), dim3(grid), dim3(64), lds, s, a);
    else if (q8 && perq)
        hipLaunchKernelGGL((hnsw_search_kernel<SPILL, true, true>), dim3(grid), dim3(64), lds, s, a);
    else if (q8)
        hipLaunchKernelGGL((hnsw_search_kernel<SPILL, true, false>), dim3(grid), dim3(64), lds, s, a);
    else if (perq)
        hipLaunchKernelGGL((hnsw_search_kernel<SPILL, false, true>), dim3(grid), dim3(64), lds, s, a);
    else
        hipLaunchKernelGGL((hnsw_search_kernel<SPILL, false, false>), dim3(grid), dim3(64), lds, s, a);
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
};

uint32_t results_need(uint32_t ef_eff, uint32_t n) { return std::min<uint32_t>(ef_eff, std::max<uint32_t>(n, 1)) + 1; }
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
    const uint32_t ccap = cand_cap(w.ef_lds, h->lds_ccap, w.qkind == 1 || w.qkind == 3 ? qlds : h->dim, n);
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
        HN_TRY(hipMemsetAsync(sc->vis.p, 0, (size_t)nb * vwords * 4, s));
        const size_t fixed = (size_t)qlds * 4 + 32 * 4 + 32 * 4 + 4 * 4;
        if (nl) {
            HN_TRY(hipMemsetAsync(a.flags, 0, (size_t)nl * 4, s));
            a.nq = nl;
            a.rcap = w.rcap_lds;
            a.ccap = ccap;
            const size_t lds = fixed + ((size_t)a.rcap + a.ccap) * sizeof(Ent);
            launch_walk<false>(q8, bin, perq, w.qkind, mix, nl, lds, s, a);
            HN_TRY(hipGetLastError());
        }
        if (nl < nb)  // results heaps no wave can keep in LDS: these queries go straight to the spill launch
            HN_TRY(hipMemsetD32Async((hipDeviceptr_t)(a.flags + nl), 1, nb - nl, s));
        a.nq = nb;
        a.rcap = s_rcap;
        a.ccap = s_ccap;
        launch_walk<true>(q8, bin, perq, w.qkind, mix, std::min(regions, nb), fixed, s, a);
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

// What a Binary-storage handle does not serve (docs/hnsw.md §18): refused before anything is written or enqueued.
nmn_status refuse_binary(const nmn_hnsw* h, const char* entry, const char* why) {
    if (h->storage != NMN_HNSW_STORAGE_BINARY) return NMN_OK;
    char buf[256];
    snprintf(buf, sizeof buf, "HNSW: %s is not served on a handle with Binary storage (%s)", entry, why);
    return set_error(NMN_ERR_CONFIGURATION, buf);
}
constexpr const char* kBinNoRows = "it keeps one bit per dimension and no f32 rows on the device";
constexpr const char* kBinQueries = "Binary rows are walked with dense queries only";
constexpr const char* kBinNodes = "a binary handle holds Binary nodes only";

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

nmn_status check_cfg(const nmn_hnsw_config* c) {
    if (c->storage != NMN_HNSW_STORAGE_DENSE)
        return set_error(NMN_ERR_CONFIGURATION, "HNSW: only HNSWStorageStrategy::Dense is served (Auto / Quantized are out of scope)");
    if (c->distance_metric < NMN_METRIC_COSINE || c->distance_metric > NMN_METRIC_DOT_PRODUCT)
        return set_error(NMN_ERR_CONFIGURATION, "HNSW: distance_metric must be Cosine, Euclidean or DotProduct");
    if (c->m == 0 || c->m0 == 0 || c->m > 4096 || c->m0 > 4096) return set_error(NMN_ERR_CONFIGURATION, "HNSW: m / m0 out of range");
    return NMN_OK;
}

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

namespace {
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
}  // namespace

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
    }
    for (DevBuf* b : {&h->d_l0, &h->d_l0cnt, &h->d_upidx, &h->d_up, &h->d_upcnt, &h->d_nrec, &h->d_nent, &h->d_live, &h->bk_lv, &h->bk_vis, &h->bk_out, &h->bk_patch, &h->hq, &h->hids, &h->hsc, &h->hcnt, &h->hkef,
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
    if (h->storage != NMN_HNSW_STORAGE_DENSE || h->n_sparse || !h->vectors) return false;
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
    hipLaunchKernelGGL(hnsw_insert_walk_kernel, dim3(nb), dim3(64), lds, s, a);
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
    hipLaunchKernelGGL(hnsw_patch_kernel, dim3((uint32_t)std::min<size_t>(nrec, 65535)), dim3(64), 0, s, a);
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

// nmn_hnsw_insert, nmn_hnsw_insert_sparse and nmn_hnsw_insert_auto behind their argument checks.  rows_host: the n rows as the
// flat index keeps them (to_dense() of a Sparse node).  sp / sp_row (dense handle only, nullable): row i is EmbeddingStorage::Sparse
// with the entries of sp's vector sp_row[i] when sp_row[i] >= 0, Dense otherwise.
nmn_status insert_rows(nmn_hnsw* h, const float* rows_host, uint64_t n, const SparseQueries* sp, const int64_t* sp_row,
                       uint64_t* ids_out, bool bulk = false) {
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
        } else if (!q8 && !bin) {
            const float* v = h->rows.data() + (have + i) * dim;
            h->mags.push_back(sqrtf(h_dot8(v, v, dim)));  // simd::magnitude, hnsw.rs:198-229
        }
        host_insert_node(h, (uint32_t)(have + i), vis);
        if (ids_out) ids_out[i] = have + i;
    }
    return upload_graph(h);
}

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
        out->sparse_count = h->n_sparse;
        out->dense_count = n - h->n_sparse;
        out->embedding_bytes = (n - h->n_sparse) * 4ull * h->dim + h->n_sparse * 56ull + 8ull * h->sp_pos.size();
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
    auto hand_out = [&]() -> nmn_status {  // the rows of every caller, top_k apart, to its own buffers
        uint32_t o = 0;
        for (const HostWalk* r : batch) {
            HN_TRY(hipMemcpyAsync(r->out_ids, (uint64_t*)h->hids.p + (size_t)o * top_k, (size_t)r->nq * top_k * 8, hipMemcpyDeviceToHost, s));
            HN_TRY(hipMemcpyAsync(r->out_scores, (float*)h->hsc.p + (size_t)o * top_k, (size_t)r->nq * top_k * 4, hipMemcpyDeviceToHost, s));
            HN_TRY(hipMemcpyAsync(r->out_counts, (uint32_t*)h->hcnt.p + o, (size_t)r->nq * 4, hipMemcpyDeviceToHost, s));
            o += r->nq;
        }
        return NMN_OK;
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
    if ((st = hand_out()) != NMN_OK) return st;
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
        if ((st = hand_out()) != NMN_OK) return st;
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
        uint32_t off = 0;
        for (const HostWalk* r : batch) {
            HN_TRY(hipMemcpyAsync(r->out_ids, (uint64_t*)h->hids.p + (size_t)off * k0, (size_t)r->nq * k0 * 8, hipMemcpyDeviceToHost, s));
            HN_TRY(hipMemcpyAsync(r->out_scores, (float*)h->hsc.p + (size_t)off * k0, (size_t)r->nq * k0 * 4, hipMemcpyDeviceToHost, s));
            HN_TRY(hipMemcpyAsync(r->out_counts, (uint32_t*)h->hcnt.p + off, (size_t)r->nq * 4, hipMemcpyDeviceToHost, s));
            off += r->nq;
        }
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

}  // namespace

extern "C" nmn_status nmn_hnsw_search(nmn_hnsw* h, const float* queries, uint32_t nq, uint32_t k, uint32_t ef, uint64_t* out_ids,
                                      float* out_scores, uint32_t* out_counts, nmn_search_stats* stats) {
    if (!h) return set_error(NMN_ERR_INVALID_ARGUMENT, "null argument");
    if (k == 0) return set_error(NMN_ERR_INVALID_TOP_K, "k == 0");
    if (stats) {
        memset(stats, 0, sizeof *stats);
        stats->scan_ms = stats->total_ms = -1.0f;
    }
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
    if (stats) {
        memset(stats, 0, sizeof *stats);
        stats->scan_ms = stats->total_ms = -1.0f;
    }
    if (nq == 0) return NMN_OK;
    if (!queries || !k || !out_ids || !out_scores || !out_counts) return set_error(NMN_ERR_INVALID_ARGUMENT, "null argument");
    for (uint32_t i = 0; i < nq; i++) {  // before the call joins a batch: a bad call fails alone, and nothing is written
        if (k[i] == 0) return set_error(NMN_ERR_INVALID_TOP_K, "k == 0");
        if (k[i] > kstride) return set_error(NMN_ERR_INVALID_ARGUMENT, "HNSW: k[i] above kstride, the row stride of the outputs");
    }
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
    if (stats) {
        memset(stats, 0, sizeof *stats);
        stats->scan_ms = stats->total_ms = -1.0f;
    }
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
    if (stats) {
        memset(stats, 0, sizeof *stats);
        stats->scan_ms = stats->total_ms = -1.0f;
    }
    if (nq == 0) return NMN_OK;
    if (!indptr || !k || !out_ids || !out_scores || !out_counts) return set_error(NMN_ERR_INVALID_ARGUMENT, "null argument");
    for (uint32_t i = 0; i < nq; i++) {  // before the call joins a batch: a bad call fails alone, and nothing is written
        if (k[i] == 0) return set_error(NMN_ERR_INVALID_TOP_K, "k == 0");
        if (k[i] > kstride) return set_error(NMN_ERR_INVALID_ARGUMENT, "HNSW: k[i] above kstride, the row stride of the outputs");
    }
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
    std::shared_lock<std::shared_mutex> g(h->rw);
    const uint64_t c64 = metric_candidates(h, top_k);
    const uint32_t c = (uint32_t)c64;
    HN_TRY(hipSetDevice(h->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    nmn_hnsw::Scratch* sc = scratch_of(h, s);
    {
        std::lock_guard<std::mutex> slk(sc->mu);  // grow, walk, re-rank and ordering as one unit on this stream
        st = metric_scratch(sc, s, nq, c, top_k);
        if (st != NMN_OK) return st;
        st = enqueue_search_locked(h, sc, queries_dev, nq, c, 0, (uint64_t*)sc->xids.p, (float*)sc->xsc.p, (uint32_t*)sc->xcnt.p, s);
        if (st != NMN_OK) return st;
        st = enqueue_rerank(h, sc, queries_dev, nq, c, top_k, *metric, out_ids_dev, out_scores_dev, out_counts_dev, s);
        if (st != NMN_OK) return st;
    }
    return record_search(h, s);
}

extern "C" nmn_status nmn_hnsw_search_metric(nmn_hnsw* h, const float* queries, uint32_t nq, uint32_t top_k, const nmn_xmetric* metric,
                                             uint64_t* out_ids, float* out_scores, uint32_t* out_counts, nmn_search_stats* stats) {
    nmn_status st = check_metric_call(h, top_k, metric);
    if (st != NMN_OK) return st;
    if (stats) {
        memset(stats, 0, sizeof *stats);
        stats->scan_ms = stats->total_ms = -1.0f;
    }
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
    if (stats) {
        memset(stats, 0, sizeof *stats);
        stats->scan_ms = stats->total_ms = -1.0f;
    }
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
void clear_stats(nmn_search_stats* stats) {
    if (!stats) return;
    memset(stats, 0, sizeof *stats);
    stats->scan_ms = stats->total_ms = -1.0f;
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
    std::shared_lock<std::shared_mutex> g(h->rw);
    const uint32_t c = (uint32_t)cache_candidates(h, k);
    HN_TRY(hipSetDevice(h->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    nmn_hnsw::Scratch* sc = scratch_of(h, s);
    const XmetricFilter flt = cache_filter(h, threshold);
    {
        std::lock_guard<std::mutex> slk(sc->mu);  // grow, walk, both re-ranks and the ordering as one unit on this stream
        st = metric_scratch(sc, s, nq, c, k, true);
        if (st != NMN_OK) return st;
        st = enqueue_search_locked(h, sc, queries_dev, nq, c, 0, (uint64_t*)sc->xids.p, (float*)sc->xsc.p, (uint32_t*)sc->xcnt.p, s);
        if (st != NMN_OK) return st;
        st = enqueue_rerank(h, sc, queries_dev, nq, c, k, *metric, out_ids_dev, out_scores_dev, out_counts_dev, s, &flt);
        if (st != NMN_OK) return st;
    }
    return record_search(h, s);
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

// ---- tensor-train queries and insert_tt_vector (hnsw.rs:1196-1221, 1755-1759, 1811-1903, 2238-2272; docs/hnsw.md §17) ---------------
namespace {

// cosine_distance_tt_with_norm on a node that is not stored as TT (hnsw.rs:1210-1219): q = tt_reconstruct(query), qmag = the
// walk's magnitude of the query (tt_norm, 0.0 when it is below 1e-10: the `== 0.0` tests below then return the reference's 1.0).
// Dense: simd::dot_product and simd::magnitude; Sparse: dot_dense and SparseVector::magnitude(); Quantized: dot_dense and
// magnitude_immutable — Cosine on every handle.
inline float tt_node_distance(const nmn_hnsw* h, uint32_t node, const float* q, float qmag, float qsum) {
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
void host_search_one_tt(const nmn_hnsw* h, const float* q, float norm, uint32_t k, uint64_t ef, HostVisited& vis, uint64_t* ids,
                        float* scores, uint32_t* count, uint64_t* evals) {
    const float qmag = tt_walk_magnitude(norm);
    const float qsum = h->storage == NMN_HNSW_STORAGE_QUANTIZED ? h_sum8(q, h->dim) : 0.0f;
    host_walk_one(h, [&](uint32_t node) { return tt_node_distance(h, node, q, qmag, qsum); }, k, ef, vis, ids, scores, count, evals,
                  NMN_METRIC_COSINE);
}

// The walk of nq prepared TT queries on s: q_dev [nq][dim] the reconstructions, mag_dev [nq] their magnitudes.  The kernel already
// knows "a dense query whose Cosine magnitude is given": kind 2.  A quantized handle takes the QK = 2 launch; a handle with Sparse
// nodes the MIX launch with kind 2 for every query (mix_dense_query with the given magnitude), under every metric of the handle;
// a dense handle the per-query form QK = 3 on dense rows with a kind array of 2s (entries = false, mag_given = true) — no
// instantiation is added.  Caller holds rw (shared) and sc->mu.
nmn_status enqueue_tt_walk_locked(nmn_hnsw* h, nmn_hnsw::Scratch* sc, const float* q_dev, const float* mag_dev, uint32_t nq, uint32_t k,
                                  uint32_t ef, uint64_t* o_ids, float* o_sc, uint32_t* o_cnt, hipStream_t s) {
    WalkShape w = uniform_shape(h, nq, k, ef);
    w.cosine = true;
    w.qmag = mag_dev;
    if (h->storage == NMN_HNSW_STORAGE_QUANTIZED || h->n_sparse > 0) {
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
    if (stats) {
        memset(stats, 0, sizeof *stats);
        stats->scan_ms = stats->total_ms = -1.0f;
    }
    if (nq == 0) return NMN_OK;
    if (!core_off || !out_ids || !out_scores || !out_counts) return set_error(NMN_ERR_INVALID_ARGUMENT, "null argument");
    TTBatch b;
    nmn_status st = tt_check(shape, n_cores, ranks, true, core_off, nq, true, &b);
    if (st != NMN_OK) return st;
    if (core_off[nq] > core_off[0] && !cores) return set_error(NMN_ERR_INVALID_ARGUMENT, "null argument");
    if ((st = tt_dim_check(h, b)) != NMN_OK) return st;
    b.cores = cores;
    const bool on_host = host_search_forced();
    const uint32_t dim = h->dim;
    uint64_t evals = 0;
    uint32_t spilled = 0;
    static thread_local HostVisited vis;
    std::vector<float> hrow(dim);
    auto host_one = [&](uint32_t q) {  // preparation and walk of train q on the host, into the caller's row
        tt_reconstruct_host(shape, n_cores, b.ranks_of(q), cores + core_off[q], hrow.data());
        const float norm = tt_norm_host(shape, n_cores, b.ranks_of(q), cores + core_off[q]);
        host_search_one_tt(h, hrow.data(), norm, k, ef ? ef : h->cfg.ef_search, vis, out_ids + (size_t)q * k, out_scores + (size_t)q * k,
                           out_counts + q, &evals);
    };
    std::shared_lock<std::shared_mutex> g(h->rw);
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
            st = enqueue_tt_walk_locked(h, sc, (const float*)sc->ttq.p, (const float*)sc->ttmag.p, nq, k, ef, (uint64_t*)h->hids.p,
                                        (float*)h->hsc.p, (uint32_t*)h->hcnt.p, s);
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
                                    out_counts_dev, s);
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

// ---- persistence (docs/hnsw.md §10) ----------------------------------------------------------------------------------------------
// File = PersistHeader{kind = hnsw, flags bit 0 = quantized, rows = n, aux = graph bytes, reserved = FNV-1a 64 of the graph section}
// | graph section (config, rng, entry, max_layer, n_upper, levels, layer-0 counts, layer-0 ids, upper lists) | rows section.
// No kernel of its own: a load is sequential reads, host checks and bulk copies.  Nothing of a file reaches hnsw_search_kernel
// before the host has proved every id of it in bounds (a neighbour id >= n, or a level-0 node listed on an upper layer, whose up_idx
// is kNone, would be an out-of-bounds read on the device).
#include "nmn_persist.h"

static_assert(sizeof(nmn_hnsw_config) == 48, "nmn_hnsw_config is part of the file format");

static const char* const kSaveSparseRefusal =
    "HNSW: the index holds sparse nodes (nmn_hnsw_insert_sparse / nmn_hnsw_insert_auto) and index file format version 1 has no place "
    "for their stored entries; saving it would lose them";

namespace {

constexpr uint64_t kGraphFixed = 48 + 8 + 8 + 4 + 4;  // config, rng, entry_point, max_layer, n_upper

uint64_t fnv1a64(const uint8_t* p, size_t n) {
    uint64_t hsh = 0xcbf29ce484222325ull;
    for (size_t i = 0; i < n; i++) hsh = (hsh ^ p[i]) * 0x100000001b3ull;
    return hsh;
}

template <typename T>
void put(std::vector<uint8_t>& b, const T& v) {
    const uint8_t* p = reinterpret_cast<const uint8_t*>(&v);
    b.insert(b.end(), p, p + sizeof(T));
}

nmn_status bad_file(const std::string& what) { return set_error(NMN_ERR_SERIALIZATION, ("HNSW index file: " + what).c_str()); }

// a cursor over the graph section: every read is checked against the section's end
struct Cursor {
    const uint8_t* p;
    uint64_t left;
    template <typename T>
    bool get(T* out) {
        if (left < sizeof(T)) return false;
        memcpy(out, p, sizeof(T));
        p += sizeof(T);
        left -= sizeof(T);
        return true;
    }
};

// one neighbour list: count <= cap, ids < n, strictly ascending, every id of level >= layer
nmn_status read_list(Cursor& c, uint32_t count, uint32_t n, uint32_t layer, const std::vector<uint8_t>& level, uint32_t node,
                     std::vector<uint32_t>* out) {
    if ((uint64_t)count * 4 > c.left) return bad_file("graph section truncated (neighbour ids)");
    out->resize(count);
    if (count) memcpy(out->data(), c.p, (size_t)count * 4);
    c.p += (size_t)count * 4;
    c.left -= (uint64_t)count * 4;
    for (uint32_t i = 0; i < count; i++) {
        const uint32_t id = (*out)[i];
        const std::string at = " (node " + std::to_string(node) + ", layer " + std::to_string(layer) + ")";
        if (id >= n) return bad_file("neighbour id " + std::to_string(id) + " out of range" + at);
        if (i && id <= (*out)[i - 1]) return bad_file("neighbour list not strictly ascending" + at);
        if (level[id] < layer) return bad_file("neighbour id " + std::to_string(id) + " does not reach the layer it is listed on" + at);
    }
    return NMN_OK;
}

}  // namespace

namespace nmn {

nmn_status persist_write_hnsw(nmn_hnsw* h, FILE* fp, const char* path) {
    std::shared_lock<std::shared_mutex> g(h->rw);  // searches may run, inserts wait
    if (h->n_sparse) return set_error(NMN_ERR_CONFIGURATION, kSaveSparseRefusal);
    const uint64_t n = h->level.size();
    const uint32_t dim = h->dim;
    const bool q8 = h->storage == NMN_HNSW_STORAGE_QUANTIZED;
    std::vector<uint8_t> sec;
    nmn_hnsw_config cfg = h->cfg;
    cfg.storage = h->storage;
    cfg.reserved = 0;
    put(sec, cfg);
    put(sec, h->rng);
    put(sec, n ? h->entry : ~0ull);
    put(sec, h->max_layer);
    uint32_t n_upper = 0;
    for (uint8_t l : h->level) n_upper += l > 0 ? 1u : 0u;
    put(sec, n_upper);
    sec.insert(sec.end(), h->level.begin(), h->level.end());
    sec.resize((sec.size() + 3) & ~(size_t)3, 0);
    for (uint64_t i = 0; i < n; i++) put(sec, (uint32_t)h->nbr[i][0].size());
    for (uint64_t i = 0; i < n; i++)
        for (uint32_t id : h->nbr[i][0]) put(sec, id);
    for (uint64_t i = 0; i < n; i++)
        for (uint32_t l = 1; l <= h->level[i]; l++) {
            put(sec, (uint32_t)h->nbr[i][l].size());
            for (uint32_t id : h->nbr[i][l]) put(sec, id);
        }
    PersistHeader hd{};
    memcpy(hd.magic, "NMNIDX\0\1", 8);
    hd.version = 1;
    hd.kind = kPersistHnsw;
    hd.dim = dim;
    hd.flags = q8 ? 1u : 0u;
    hd.rows = n;
    hd.row_base = 0;
    hd.aux = sec.size();
    hd.reserved = fnv1a64(sec.data(), sec.size());
    uint64_t rows_bytes = 0;
    if (n) rows_bytes = q8 ? n * dim + n * 16ull : sizeof(PersistHeader) + n * dim * 4ull + n * 4ull;
    hd.payload_bytes = hd.aux + rows_bytes;
    if (fwrite(&hd, sizeof hd, 1, fp) != 1 || fwrite(sec.data(), 1, sec.size(), fp) != sec.size())
        return persist_io_error("cannot write", path);
    if (n == 0) return NMN_OK;
    if (!q8)  // the handle's flat index, from the host's copy of it: the same rows, the same magnitudes, no device traffic
        return persist_write_rows_host(fp, path, dim, n, 0, h->rows.data(), h->mags.data());
    std::vector<float> rec((size_t)n * 4);
    for (uint64_t i = 0; i < n; i++) {
        rec[4 * i + 0] = h->qscale[i];
        rec[4 * i + 1] = h->qmin[i];
        rec[4 * i + 2] = h->mags[i];
        rec[4 * i + 3] = h->qxsq[i];
    }
    if (fwrite(h->codes.data(), dim, n, fp) != n || fwrite(rec.data(), 16, n, fp) != n) return persist_io_error("cannot write", path);
    return NMN_OK;
}

// the file persist_write_hnsw wrote, header already read into hd (persist_read_header: magic, version, payload within the file)
nmn_status persist_read_hnsw(FILE* fp, const char* path, const PersistHeader& hd, int32_t device, uint64_t capacity_hint,
                             nmn_hnsw** out) {
    *out = nullptr;
    if (hd.kind != kPersistHnsw) return bad_file("not an HNSW index file (another kind of section)");
    if (hd.dim == 0 || hd.dim > kMaxDim) return bad_file("dimension out of range (1 .. 8192)");
    if (hd.flags & ~1u) return bad_file("unknown flag bits");
    if (hd.row_base != 0) return bad_file("row_base must be 0");
    const bool q8 = (hd.flags & 1u) != 0;
    const uint32_t dim = hd.dim;
    // sizes: everything announced must be in the file before it sizes anything
    const uint64_t left = persist_bytes_left(fp);
    if (left == UINT64_MAX) return set_error(NMN_ERR_IO, "IO error: cannot seek in the index file");
    if (hd.payload_bytes != left) return bad_file("payload_bytes differs from the bytes that follow the header");
    if (hd.aux > hd.payload_bytes || hd.aux < kGraphFixed) return bad_file("graph section size is inconsistent with the file");
    if (hd.rows > hd.aux / 4 || hd.rows >= (uint64_t)kNone) return bad_file("node count is inconsistent with the graph section size");
    const uint64_t n64 = hd.rows;
    const uint32_t n = (uint32_t)n64;
    {
        unsigned __int128 rows_bytes = 0;
        if (n64) rows_bytes = q8 ? (unsigned __int128)n64 * dim + (unsigned __int128)n64 * 16
                                 : (unsigned __int128)sizeof(PersistHeader) + (unsigned __int128)n64 * dim * 4 + (unsigned __int128)n64 * 4;
        if ((unsigned __int128)hd.aux + rows_bytes != (unsigned __int128)hd.payload_bytes)
            return bad_file("payload_bytes is inconsistent with the node count and the dimension");
    }
    std::vector<uint8_t> sec((size_t)hd.aux);
    if (fread(sec.data(), 1, sec.size(), fp) != sec.size()) return bad_file("truncated (graph section)");
    if (fnv1a64(sec.data(), sec.size()) != hd.reserved) return bad_file("corrupt: graph section checksum mismatch");
    Cursor c{sec.data(), hd.aux};
    nmn_hnsw_config cfg;
    uint64_t rng = 0, entry = 0;
    uint32_t max_layer = 0, n_upper = 0;
    (void)c.get(&cfg);  // (aux >= kGraphFixed)
    (void)c.get(&rng);
    (void)c.get(&entry);
    (void)c.get(&max_layer);
    (void)c.get(&n_upper);
    if (cfg.storage == NMN_HNSW_STORAGE_AUTO) return bad_file("config storage is Auto, which no handle has");
    if (cfg.storage != (q8 ? NMN_HNSW_STORAGE_QUANTIZED : NMN_HNSW_STORAGE_DENSE)) return bad_file("config storage differs from the header's flag");
    if (cfg.reserved != 0) return bad_file("config reserved field is not 0");
    nmn_hnsw_config cfg_dense = cfg;
    cfg_dense.storage = NMN_HNSW_STORAGE_DENSE;  // (check_cfg and create_handle take the strategy apart from the config)
    if (check_cfg(&cfg_dense) != NMN_OK) return bad_file(std::string("invalid config: ") + nmn_last_error());
    if (cfg.max_nodes > 0 && n64 > cfg.max_nodes) return bad_file("more nodes than the config's max_nodes");
    if (rng == 0) return bad_file("rng state is 0 (the xorshift generator never reaches it)");
    if (n == 0) {
        if (entry != ~0ull || max_layer != 0 || n_upper != 0) return bad_file("an empty index with an entry point, a layer or upper nodes");
    } else if (entry >= n64) {
        return bad_file("entry point out of range");
    }
    // levels, zero-padded to 4 bytes
    const uint64_t lv_bytes = ((uint64_t)n + 3) & ~3ull;
    if (lv_bytes > c.left) return bad_file("graph section truncated (levels)");
    std::vector<uint8_t> level(c.p, c.p + n);
    for (uint64_t i = n; i < lv_bytes; i++)
        if (c.p[i] != 0) return bad_file("level padding is not zero");
    c.p += lv_bytes;
    c.left -= lv_bytes;
    uint32_t top = 0, upper = 0;
    for (uint32_t i = 0; i < n; i++) {
        if (level[i] > 32) return bad_file("level of node " + std::to_string(i) + " above 32");
        top = std::max<uint32_t>(top, level[i]);
        upper += level[i] > 0 ? 1u : 0u;
    }
    if (n) {
        if (max_layer != top) return bad_file("max_layer differs from the highest level");
        if (level[entry] != max_layer) return bad_file("the entry point's level is not max_layer");
        if (n_upper != upper) return bad_file("n_upper differs from the count of nodes of level >= 1");
    }
    // layer 0: counts, then the lists
    if ((uint64_t)n * 4 > c.left) return bad_file("graph section truncated (layer-0 counts)");
    std::vector<uint32_t> l0cnt(n);
    if (n) memcpy(l0cnt.data(), c.p, (size_t)n * 4);
    c.p += (size_t)n * 4;
    c.left -= (uint64_t)n * 4;
    for (uint32_t i = 0; i < n; i++)
        if (l0cnt[i] > cfg.m0) return bad_file("layer-0 count of node " + std::to_string(i) + " above m0");
    std::vector<std::vector<std::vector<uint32_t>>> nbr(n);
    nmn_status st = NMN_OK;
    for (uint32_t i = 0; i < n; i++) {
        nbr[i].resize((size_t)level[i] + 1);
        st = read_list(c, l0cnt[i], n, 0, level, i, &nbr[i][0]);
        if (st != NMN_OK) return st;
    }
    for (uint32_t i = 0; i < n; i++)
        for (uint32_t l = 1; l <= level[i]; l++) {
            uint32_t cnt = 0;
            if (!c.get(&cnt)) return bad_file("graph section truncated (upper-layer count)");
            if (cnt > cfg.m) return bad_file("upper-layer count of node " + std::to_string(i) + " above m");
            st = read_list(c, cnt, n, l, level, i, &nbr[i][l]);
            if (st != NMN_OK) return st;
        }
    if (c.left != 0) return bad_file("trailing bytes in the graph section");
    sec.clear();
    sec.shrink_to_fit();

    // rows: read and proved on the host
    std::vector<float> rows, mags, qscale, qmin, qxsq;
    std::vector<uint8_t> codes;
    if (n && !q8) {
        PersistHeader hv{};
        st = persist_read_header(fp, path, &hv);
        if (st != NMN_OK) return st;
        if (hv.kind != kPersistFlat || hv.dim != dim || hv.rows != n64 || hv.row_base != 0 ||
            hv.payload_bytes != n64 * dim * 4ull + n64 * 4ull)
            return bad_file("the rows section's header is inconsistent with the index");
        st = persist_read_rows_host(fp, hv, &rows, &mags);  // (its checksum)
        if (st != NMN_OK) return st;
        for (uint32_t i = 0; i < n; i++) {
            const float* v = rows.data() + (size_t)i * dim;
            const float m = sqrtf(h_dot8(v, v, dim));
            if (memcmp(&m, &mags[i], 4) != 0) return bad_file("corrupt: row magnitudes differ from the stored ones (row " + std::to_string(i) + ")");
        }
    } else if (n) {
        codes.resize((size_t)n * dim);
        std::vector<float> rec((size_t)n * 4);
        if (fread(codes.data(), dim, n, fp) != n || fread(rec.data(), 16, n, fp) != n) return bad_file("truncated (quantized rows)");
        rows.resize((size_t)n * dim);
        mags.resize(n);
        qscale.resize(n);
        qmin.resize(n);
        qxsq.resize(n);
        for (uint32_t i = 0; i < n; i++) {
            qscale[i] = rec[4 * (size_t)i + 0];
            qmin[i] = rec[4 * (size_t)i + 1];
            const uint8_t* code = codes.data() + (size_t)i * dim;
            float* v = rows.data() + (size_t)i * dim;
            h_dequantize(code, dim, qscale[i], qmin[i], v);
            mags[i] = sqrtf(h_dot8(v, v, dim));
            qxsq[i] = h_q8_sqmag(code, qscale[i], qmin[i], dim);
            if (memcmp(&mags[i], &rec[4 * (size_t)i + 2], 4) != 0 || memcmp(&qxsq[i], &rec[4 * (size_t)i + 3], 4) != 0)
                return bad_file("corrupt: quantized row " + std::to_string(i) + " does not give its stored magnitude / squared magnitude");
        }
    }
    if (persist_bytes_left(fp) != 0) return bad_file("trailing bytes after the rows section");

    // the handle: device arrays sized by numbers the checks above have bounded by the file's size
    nmn_hnsw* h = nullptr;
    st = create_handle(&cfg_dense, q8 ? NMN_HNSW_STORAGE_QUANTIZED : NMN_HNSW_STORAGE_DENSE, dim, std::max<uint64_t>(capacity_hint, n64),
                       device, &h);
    if (st != NMN_OK) return st;
    auto fail_with = [&](nmn_status s) {
        const std::string keep = nmn_last_error();
        nmn_hnsw_destroy(h);
        return set_error(s, keep.c_str());
    };
    h->rows = std::move(rows);
    h->mags = std::move(mags);
    h->codes = std::move(codes);
    h->qscale = std::move(qscale);
    h->qmin = std::move(qmin);
    h->qxsq = std::move(qxsq);
    h->level = std::move(level);
    h->nbr = std::move(nbr);
    h->entry = n ? entry : ~0ull;
    h->max_layer = max_layer;
    h->rng = rng;
    if (n && !q8) {
        st = nmn_index_upload(h->vectors, h->rows.data(), 0, n64);  // H2D + the magnitudes in reference order, on the device
        if (st != NMN_OK) return fail_with(st);
        std::vector<float> got(n);
        const hipError_t e = hipMemcpy(got.data(), h->vectors->norms, (size_t)n * 4, hipMemcpyDeviceToHost);
        if (e != hipSuccess) return fail_with(set_error_hip(e, "reading the magnitudes back"));
        if (memcmp(got.data(), h->mags.data(), (size_t)n * 4) != 0)
            return fail_with(bad_file("corrupt: the device's row magnitudes differ from the stored ones"));
    } else if (n) {
        st = upload_codes(h, 0, n64);
        if (st != NMN_OK) return fail_with(st);
    }
    st = upload_graph(h);
    if (st != NMN_OK) return fail_with(st);
    *out = h;
    return NMN_OK;
}

}  // namespace nmn

extern "C" nmn_status nmn_hnsw_get_config(const nmn_hnsw* h, nmn_hnsw_config* out) {
    if (!h || !out) return set_error(NMN_ERR_INVALID_ARGUMENT, "null argument");
    *out = h->cfg;
    out->storage = h->storage;
    out->reserved = 0;
    return NMN_OK;
}

extern "C" nmn_status nmn_hnsw_save(nmn_hnsw* h, const char* path) {
    if (!h || !path) return set_error(NMN_ERR_INVALID_ARGUMENT, "null argument");
    if (const nmn_status sb = refuse_binary(h, "nmn_hnsw_save", "the file format has no Binary rows section yet"); sb != NMN_OK) return sb;
    {
        std::shared_lock<std::shared_mutex> g(h->rw);
        if (h->n_sparse) return set_error(NMN_ERR_CONFIGURATION, kSaveSparseRefusal);  // before the file is touched
    }
    FILE* fp = fopen(path, "wb");
    if (!fp) return persist_io_error("cannot create", path);
    nmn_status st = persist_write_hnsw(h, fp, path);
    if (fclose(fp) != 0 && st == NMN_OK) st = persist_io_error("cannot close", path);
    return st;
}

extern "C" nmn_status nmn_hnsw_load(const char* path, int32_t device, uint64_t capacity_hint, uint64_t max_file_bytes,
                                    uint64_t max_entries, nmn_hnsw** out) {
    if (!path || !out) return set_error(NMN_ERR_INVALID_ARGUMENT, "null argument");
    *out = nullptr;
    nmn_status st = persist_check_file_size(path, max_file_bytes, nullptr);
    if (st != NMN_OK) return st;
    FILE* fp = fopen(path, "rb");
    if (!fp) return persist_io_error("cannot open", path);
    PersistHeader hd{};
    st = persist_read_header(fp, path, &hd);
    if (st == NMN_OK) st = persist_check_entries(hd.rows, max_entries);
    if (st == NMN_OK) st = persist_read_hnsw(fp, path, hd, device, capacity_hint, out);
    fclose(fp);
    return st;
}
