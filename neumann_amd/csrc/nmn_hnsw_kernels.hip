// nmn_hnsw_kernels.hip — the device side of the HNSW index (docs/hnsw.md): the device distances, hnsw_search_kernel (one query
// per wave, the whole walk in one launch), hnsw_insert_walk_kernel and hnsw_patch_kernel of the bulk build (§19), and their
// launchers.  The only translation unit of the index with __global__ code; the kernels are launched from here alone.
// THIS TRANSLATION UNIT IS BUILT WITH -ffp-contract=off -fhip-fp32-correctly-rounded-divide-sqrt (build.py), host and device:
// every distance restates the reference's unfused f32 arithmetic and must give its bits (docs/hnsw.md, "Source layout").
#include "nmn_hnsw_kernels.h"
#include "nmn_internal.h"
#include "nmn_tt.h"

#pragma clang fp contract(off)

namespace nmn {
namespace {

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
// TTN (dense rows, PERQ, QK == 3, every query of kind 2; docs/hnsw.md §24): the queries are TTVectors and the handle holds
// EmbeddingStorage::TensorTrain nodes.  Such a node is scored by cosine_distance_tt_with_norm's first arm (hnsw.rs:1201-1209):
// tt_dot_product(node, query) — node first — over the product of the cached norms, nothing reconstructed.  The query's ranks and
// cores sit in LDS in front of the heaps, beside its reconstruction (which every other node is still scored with), with two Gram
// buffers.  Pair-of-lanes scoring leaves a TT node's stage slot empty; the staged TT nodes of a pass are then taken ONE AT A TIME
// by the whole wave (tt_node_distance: the 64 lanes share out the outputs of each core step, tt_gram_step's unsplit chains, a
// barrier between steps).  Which slots hold TT nodes is read from LDS and the slot array by every lane alike, so the loop and its
// barriers are wave-uniform.  The visited bitmap, both heaps, lane 0's decision loop and the final order are untouched.
template <bool SPILL, bool Q8, bool PERQ, int QK = 0, bool MIX = false, bool BIN = false, bool TTN = false>
__global__ __launch_bounds__(64) void hnsw_search_kernel(SearchArgs a) {
    static_assert(QK == 0 || (QK == 1 && !Q8 && !PERQ) || (QK == 2 && Q8 && !PERQ) || (QK == 3 && PERQ),
                  "query kinds: 1 on dense rows, 2 on quantized rows, 3 = a kind per query of a per-query launch");
    static_assert(!MIX || (!Q8 && PERQ && QK == 3), "sparse nodes: dense storage, the per-query form");
    static_assert(!BIN || (!Q8 && QK == 0 && !MIX), "binary rows: dense queries, a storage of their own");
    static_assert(!TTN || (!Q8 && PERQ && QK == 3 && !BIN), "TT nodes: dense storage, the per-query form");
    extern __shared__ float4 smem4[];
    const GraphDev& g = a.g;
    const uint32_t lane = threadIdx.x, p = lane >> 1, h = lane & 1u;
    float* qs = reinterpret_cast<float*>(smem4);
    uint32_t* stage_id = reinterpret_cast<uint32_t*>(qs + a.qlds);
    float* stage_d = reinterpret_cast<float*>(stage_id + 32);
    uint32_t* ctrl = reinterpret_cast<uint32_t*>(stage_d + 32);  // [0] done, [1] current node, [2] overflow, [3] results
    // TTN: [16] the query's ranks, [ttq_cap rounded up to 2] its cores, two Gram buffers of tt_gcap (rounded up to 2) floats
    uint32_t* tq_rank = ctrl + 4;
    float* tq_core = reinterpret_cast<float*>(tq_rank + 16);
    float* tt_gram = tq_core + ((a.ttq_cap + 1u) & ~1u);
    const uint32_t tt_gstride = (a.tt_gcap + 1u) & ~1u;
    Ent* R;
    Ent* Cn;
    if (SPILL) {
        R = a.spill + (size_t)blockIdx.x * ((size_t)a.rcap + a.ccap);
        Cn = R + a.rcap;
    } else {
        R = reinterpret_cast<Ent*>(ctrl + 4 + (TTN ? tt_region_floats(a.ttq_cap, a.tt_gcap) : 0u));
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
        if constexpr (TTN) {  // the query's ranks (checked by the host before the launch), then its cores, ttq_cap floats at most
            if (lane <= a.ttq_ncores)
                tq_rank[lane] = a.ttq_ranks ? a.ttq_ranks[(size_t)q * (a.ttq_ncores + 1u) + lane] : a.ttq_ranks_u[lane];
            __syncthreads();
            uint32_t storage = 0;
            for (uint32_t c = 0; c < a.ttq_ncores; c++) storage += tq_rank[c] * a.ttq_shape[c] * tq_rank[c + 1];
            storage = min(storage, a.ttq_cap);
            const float* src = a.ttq_cores + (a.ttq_off ? a.ttq_off[q] : (uint64_t)q * a.ttq_stride);
            for (uint32_t i = lane; i < storage; i += 64) tq_core[i] = src[i];
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
            if constexpr (TTN) {
                if (a.tt_slot[node] != kNone) return 0.0f;  // (the whole wave scores it from the stage, tt_node_distance)
            }
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
        // cosine_distance_tt_with_norm on a TensorTrain node (hnsw.rs:1196-1209), by the whole wave, `slot` the same in every lane.
        // qmag is the query's norm with a norm below 1e-10 written as 0.0 (tt_walk_magnitude): the first test.  A node of another
        // shape is tt_dot_product's Err: 1.0.  Then the Gram chain, node first; then the node's own `< 1e-10` test and the quotient.
        auto tt_node_distance = [&](uint32_t slot) -> float {
            const TTNodeDev& r = a.tt_rec[slot];
            const uint32_t nc = r.n_cores;
            bool same = nc == a.ttq_ncores && nc <= 8u;
            uint64_t need = 0;
            for (uint32_t c = 0; c < 8u; c++)
                if (same && c < nc) {
                    same = r.modes[c] == a.ttq_shape[c];
                    need += (uint64_t)r.ranks[c] * r.modes[c] * r.ranks[c + 1];
                    same = same && r.ranks[c] * tq_rank[c] <= a.tt_gcap && r.ranks[c + 1] * tq_rank[c + 1] <= a.tt_gcap;
                }
            const uint64_t off = ((uint64_t)r.off_hi << 32) | r.off_lo;
            if (qmag == 0.0f || !same || off > a.tt_pool || need > a.tt_pool - off) return 1.0f;  // (the bounds: the host's own)
            const float* A = a.tt_cores + off;
            __syncthreads();  // the readers of the previous node's Gram buffers are done
            if (lane == 0) tt_gram[0] = 1.0f;  // gram = [1.0]
            uint32_t ca = 0, cb = 0;
            for (uint32_t c = 0; c < nc; c++) {
                __syncthreads();
                const uint32_t r1a = r.ranks[c], r2a = r.ranks[c + 1], r1b = tq_rank[c], r2b = tq_rank[c + 1], m = r.modes[c];
                const uint32_t cur = c & 1u;
                tt_gram_step(A + ca, tq_core + cb, tt_gram + cur * tt_gstride, tt_gram + (cur ^ 1u) * tt_gstride, r1a, r2a, r1b, r2b, m,
                             lane);
                ca += r1a * m * r2a;
                cb += r1b * m * r2b;
            }
            __syncthreads();
            const float dot = tt_gram[(nc & 1u) * tt_gstride];
            const float nnorm = __uint_as_float(r.norm_bits);
            if (nnorm < 1e-10f) return 1.0f;
            return 1.0f - dot / (nnorm * qmag);
        };
        // the staged neighbours of one pass that are TT nodes, one at a time; every lane reads the same slots: wave-uniform
        auto tt_stage_pass = [&](uint32_t lim) {
            for (uint32_t t = 0; t < lim; t++) {
                const uint32_t id = stage_id[t];
                if (id == kNone) continue;
                const uint32_t slot = a.tt_slot[id];
                if (slot == kNone) continue;
                const float d = tt_node_distance(slot);
                if (lane == 0) stage_d[t] = d;
            }
            __syncthreads();
        };
        // distance evaluations.  The reference scores the entry of every search_layer* call again (one per greedy layer, one for
        // search_layer); this kernel carries the distance along.  A quantized or binary handle counts the evaluations the reference makes,
        // as the host walk does; a dense handle keeps the count it has always reported.
        uint32_t evals = Q8 || BIN ? g.max_layer + 1u : 1u;
        // greedy descent, hnsw.rs:2086-2092 / 2170-2200
        uint32_t cur = g.entry;
        float cur_d = row_distance(cur);
        if constexpr (TTN) {
            const uint32_t slot = a.tt_slot[cur];
            if (slot != kNone) cur_d = tt_node_distance(slot);
        }
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
                    if constexpr (TTN) tt_stage_pass(lim);
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
                if constexpr (TTN) tt_stage_pass(min(32u, cnt - j0));
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

template <bool SPILL>
void launch_walk(bool q8, bool bin, bool perq, int qkind, bool mix, bool ttn, uint32_t grid, size_t lds, hipStream_t s,
                 const SearchArgs& a) {
    if (ttn && mix)  // TT queries on a handle with TT nodes (and sparse ones): the per-query form, every query of kind 2
        hipLaunchKernelGGL((hnsw_search_kernel<SPILL, false, true, 3, true, false, true>), dim3(grid), dim3(64), lds, s, a);
    else if (ttn)
        hipLaunchKernelGGL((hnsw_search_kernel<SPILL, false, true, 3, false, false, true>), dim3(grid), dim3(64), lds, s, a);
    else if (bin && perq)  // binary rows: dense queries only (every other query form is refused before it gets here)
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

}  // namespace

namespace hnsw {

void launch_search_args(bool spill, bool q8, bool bin, bool perq, int qkind, bool mix, bool ttn, uint32_t grid, size_t lds, hipStream_t s,
                        const void* search_args) {
    const SearchArgs& a = *static_cast<const SearchArgs*>(search_args);
    if (spill)
        launch_walk<true>(q8, bin, perq, qkind, mix, ttn, grid, lds, s, a);
    else
        launch_walk<false>(q8, bin, perq, qkind, mix, ttn, grid, lds, s, a);
}
void launch_insert_walk_args(uint32_t grid, size_t lds, hipStream_t s, const void* insert_args) {
    hipLaunchKernelGGL(hnsw_insert_walk_kernel, dim3(grid), dim3(64), lds, s, *static_cast<const InsertArgs*>(insert_args));
}
void launch_patch_args(uint32_t grid, hipStream_t s, const void* patch_args) {
    hipLaunchKernelGGL(hnsw_patch_kernel, dim3(grid), dim3(64), 0, s, *static_cast<const PatchArgs*>(patch_args));
}

}  // namespace hnsw
}  // namespace nmn
