// nmn_hnsw_arith.h — what the host side and the device side of the HNSW index (docs/hnsw.md) both use, and the reference's host
// arithmetic: the constants, the heap entry, the two heaps, the f32 / quantized / binary distances of the host, cand_cap.
// Everything here has internal linkage: each translation unit that includes it compiles its own copy, inlined with its callers.
// EVERY TRANSLATION UNIT THAT INCLUDES THIS HEADER IS BUILT WITH -ffp-contract=off -fhip-fp32-correctly-rounded-divide-sqrt
// (build.py's SOURCES), host and device: every distance below restates the reference's unfused f32 arithmetic and must give its bits.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <vector>

#include "../../include/neumann_gpu.h"

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

}  // namespace
}  // namespace nmn
