// nmn_xmetric.hip — `tensor_store::DistanceMetric` (tensor_store/src/distance.rs:13-194), the ExtendedDistanceMetric of
// VectorEngine::search_with_hnsw_and_metric (vector_engine/src/lib.rs:2560-2619): the re-rank of an HNSW walk's candidates
// under any of its nine metrics, and the stable descending order of the scores.
// THIS TRANSLATION UNIT IS BUILT WITH -ffp-contract=off -fhip-fp32-correctly-rounded-divide-sqrt (build.py), host and device.
//
// Reference arithmetic restated here (docs/hnsw.md §8 has the table):
//   SparseVector::from_dense (sparse_vector.rs:221-229) stores a value iff `val != 0.0`: +-0.0 are skipped, NaN is stored.
//   dot_f64 (419-443), magnitude_f64 (553-559), cosine_similarity (583-599), angular / geodesic_distance (795-808),
//   jaccard_index (816-845), overlap_coefficient (852-878), weighted_jaccard (886-935), euclidean_distance (942-1006),
//   manhattan_distance (1013-1059): sequential f64 sums over the merged stored positions, one rounding to f32 at the end.
//   A dense left-to-right loop gives the same bits: a position neither side stores adds +0.0 to a sum that starts at 0.0 and
//   can never be -0.0 (products of two f32 are exact in f64 and never underflow), a position one side stores adds exactly what
//   the merge loop's one-sided arm adds (the missing value read as 0.0).
//   GeometricConfig::compute (distance.rs:172-193), DistanceMetric::to_similarity (92-106).
// Work split, as nmn_exact.hip's sparse_cos64: the eight lanes of a group form the terms of eight consecutive positions, and
// every lane then adds them to the f64 chains in index order.  Eight pairs to a wave.  The intersection / stored counts are
// integers and are reduced in any order.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <type_traits>
#include <vector>

#include "nmn_index.h"
#include "nmn_internal.h"

#pragma clang fp contract(off)

namespace nmn {
namespace {

constexpr uint32_t kPairsPerRound = 32;   // 256 threads, eight lanes a pair
constexpr uint32_t kPairsPerBlock = 256;  // a block serves up to eight rounds of one query: the query's constants once per block
constexpr float kPi = 3.14159274101257324f;  // std::f32::consts::PI
constexpr float kF32Max = 3.40282346638528859812e+38f;

// which f64 chains a metric needs from the one pass over the row
enum Chains : int { kChCos = 0, kChSet = 1, kChWJ = 2, kChEucl = 3, kChManh = 4, kChComposite = 5 };

__host__ __device__ inline int chains_of(int kind) {
    switch (kind) {
        case NMN_XMETRIC_COSINE:
        case NMN_XMETRIC_ANGULAR:
        case NMN_XMETRIC_GEODESIC: return kChCos;
        case NMN_XMETRIC_JACCARD:
        case NMN_XMETRIC_OVERLAP: return kChSet;
        case NMN_XMETRIC_WEIGHTED_JACCARD: return kChWJ;
        case NMN_XMETRIC_EUCLIDEAN: return kChEucl;
        case NMN_XMETRIC_MANHATTAN: return kChManh;
        default: return kChComposite;
    }
}

// f32::midpoint(a, 1.0) on x86-64: ((a as f64 + 1.0) / 2.0) as f32, one rounding
__host__ __device__ inline float midpoint1(float a) { return (float)(((double)a + 1.0) / 2.0); }

// DistanceMetric::to_similarity, distance.rs:92-106
__host__ __device__ inline float xm_to_similarity(int kind, float raw) {
    switch (kind) {
        case NMN_XMETRIC_COSINE: return midpoint1(raw);
        case NMN_XMETRIC_ANGULAR:
        case NMN_XMETRIC_GEODESIC: {
            const float t = raw / kPi;
            return 1.0f - t;
        }
        case NMN_XMETRIC_EUCLIDEAN:
        case NMN_XMETRIC_MANHATTAN: {
            const float t = 1.0f + raw;
            return 1.0f / t;
        }
        default: return raw;
    }
}

// lane T of the caller's 8-lane group to all eight (nmn_exact.hip: group8_bcast), for the two halves of an f64
template <int T>
__device__ __forceinline__ int group8_bcast_i(int v) {
    int r = __builtin_amdgcn_update_dpp(0, v, 0x150 + T, 0xF, 0x3, false);
    r = __builtin_amdgcn_update_dpp(r, v, 0x158 + T, 0xF, 0xC, false);
    return r;
}
template <int T>
__device__ __forceinline__ double group8_bcast_d(double v) {
    return __hiloint2double(group8_bcast_i<T>(__double2hiint(v)), group8_bcast_i<T>(__double2loint(v)));
}
// chain = chain + term of position 8c + 0, .., 8c + 7, in that order
__device__ __forceinline__ double chain8(double chain, double term) {
    chain = chain + group8_bcast_d<0>(term);
    chain = chain + group8_bcast_d<1>(term);
    chain = chain + group8_bcast_d<2>(term);
    chain = chain + group8_bcast_d<3>(term);
    chain = chain + group8_bcast_d<4>(term);
    chain = chain + group8_bcast_d<5>(term);
    chain = chain + group8_bcast_d<6>(term);
    chain = chain + group8_bcast_d<7>(term);
    return chain;
}
__device__ __forceinline__ uint32_t group8_sum(uint32_t v) {
    v += (uint32_t)__shfl_xor((int)v, 1);
    v += (uint32_t)__shfl_xor((int)v, 2);
    v += (uint32_t)__shfl_xor((int)v, 4);
    return v;
}

struct PairSums {
    double dot, sb, sd, man, wmin, wmax;
    uint32_t inter, nb;
};

// One pass over (query a, row b) by the eight lanes of a group, lane l owning the positions 8c + l.  Every lane returns the sums.
template <int CH>
__device__ __forceinline__ PairSums pair_pass(const float* __restrict__ a, const float* __restrict__ b, uint32_t dim, uint32_t l) {
    PairSums r{0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0u, 0u};
    constexpr int PF = 4;
    constexpr bool kDot = CH == kChCos || CH == kChComposite;
    constexpr bool kSd = CH == kChEucl || CH == kChComposite;
    const uint32_t chunks = (dim + 7u) >> 3;
    for (uint32_t c0 = 0; c0 < chunks; c0 += PF) {
        float x[PF], y[PF];
#pragma unroll
        for (int i = 0; i < PF; i++) {
            const uint32_t e = 8u * (c0 + (uint32_t)i) + l;
            x[i] = e < dim ? a[e] : 0.0f;
            y[i] = e < dim ? b[e] : 0.0f;
        }
#pragma unroll
        for (int i = 0; i < PF; i++) {
            const bool sx = x[i] != 0.0f, sy = y[i] != 0.0f;  // stored in the sparse form (true for NaN)
            const double xd = sx ? (double)x[i] : 0.0, yd = sy ? (double)y[i] : 0.0;
            r.inter += (sx && sy) ? 1u : 0u;
            r.nb += sy ? 1u : 0u;
            if (kDot) {
                r.dot = chain8(r.dot, (sx && sy) ? xd * yd : 0.0);
                r.sb = chain8(r.sb, yd * yd);
            }
            if (kSd || CH == kChManh) {
                const double d = xd - yd;
                if (kSd) r.sd = chain8(r.sd, d * d);
                if (CH == kChManh) r.man = chain8(r.man, __builtin_fabs(d));
            }
            if (CH == kChWJ) {
                const double ax = __builtin_fabs(xd), ay = __builtin_fabs(yd);
                r.wmin = chain8(r.wmin, ax < ay ? ax : ay);
                r.wmax = chain8(r.wmax, ax > ay ? ax : ay);
            }
        }
    }
    r.inter = group8_sum(r.inter);
    r.nb = group8_sum(r.nb);
    return r;
}

// cosine_similarity, sparse_vector.rs:583-599 (mag_a = sqrt of the query's sum, once per query)
__host__ __device__ inline float cos_from(double dot, double mag_a, double sb) {
    const double mag_b = __builtin_sqrt(sb);
    if (mag_a == 0.0 || mag_b == 0.0) return 0.0f;
    const double r = dot / (mag_a * mag_b);
    if (r != r || __builtin_isinf(r)) return 0.0f;
    const double c = r < -1.0 ? -1.0 : (r > 1.0 ? 1.0 : r);
    return (float)c;
}
__host__ __device__ inline float jaccard_from(uint32_t na, uint32_t nb, uint32_t inter) {  // 816-845
    if (na == 0u && nb == 0u) return 1.0f;
    if (na == 0u || nb == 0u) return 0.0f;
    return (float)inter / (float)(na + nb - inter);
}
__host__ __device__ inline float clamp_f32max(double v) {  // 943-948, 1054-1058
    return v > (double)kF32Max ? kF32Max : (float)v;
}

// DistanceMetric::compute (distance.rs:76-88) from the sums of one pass: mag_a / na are the query's magnitude_f64 and stored count
__host__ __device__ inline float finish_pair(int kind, const PairSums& s, double mag_a, uint32_t na, float cw, float sw, float mw) {
    switch (kind) {
        case NMN_XMETRIC_COSINE: return cos_from(s.dot, mag_a, s.sb);
        case NMN_XMETRIC_ANGULAR:
        case NMN_XMETRIC_GEODESIC: {  // angular_distance, 795-798: acos in f64 of the f32 cosine, rounded once
            const float c = cos_from(s.dot, mag_a, s.sb);
            const float cl = c < -1.0f ? -1.0f : (c > 1.0f ? 1.0f : c);
            return (float)acos((double)cl);
        }
        case NMN_XMETRIC_JACCARD: return jaccard_from(na, s.nb, s.inter);
        case NMN_XMETRIC_OVERLAP: {  // overlap_coefficient, 852-878
            if (na == 0u || s.nb == 0u) return 0.0f;
            return (float)s.inter / (float)(na < s.nb ? na : s.nb);
        }
        case NMN_XMETRIC_WEIGHTED_JACCARD: return s.wmax == 0.0 ? 1.0f : (float)(s.wmin / s.wmax);  // 930-934
        case NMN_XMETRIC_EUCLIDEAN: return clamp_f32max(__builtin_sqrt(s.sd));
        case NMN_XMETRIC_MANHATTAN: return clamp_f32max(s.man);
        default: {  // GeometricConfig::compute, distance.rs:172-193
            const float t0 = cw + sw;
            const float tw = t0 + mw;
            if (tw == 0.0f) return 0.0f;
            const float cosine_sim = midpoint1(cos_from(s.dot, mag_a, s.sb));
            const float jaccard_sim = jaccard_from(na, s.nb, s.inter);
            const float dist = clamp_f32max(__builtin_sqrt(s.sd));
            const float den = 1.0f + dist;
            const float euclidean_sim = 1.0f / den;
            const float m = mw * euclidean_sim;
            const float inner = __builtin_fmaf(sw, jaccard_sim, m);
            const float outer = __builtin_fmaf(cw, cosine_sim, inner);
            return outer / tw;
        }
    }
}

struct RerankArgs {
    const float* rows;      // row r at rows + r * ld
    const float* queries;   // [nq][dim]
    const uint64_t* ids;    // candidate ids: query q's at ids + q * id_stride (id_stride 0: one list for every query)
    const uint32_t* counts; // [nq] candidates of each query (nullable: c for every query)
    float* raw;             // [nq][c] compute()               (nullable)
    float* sim;             // [nq][c] to_similarity(compute()) (nullable)
    uint64_t n_rows;        // rows behind `rows`: an id at or past it is scored as NaN and never read
    uint32_t ld, dim, nq, c, id_stride;
    int kind;
    float cw, sw, mw;
};

// PERQ == true (docs/hnsw.md §12): workgroup row y serves query qsel[y] of a coalesced batch.  The candidates are read where the walk
// left them (rows kstride apart, the walk's own count), kind and weights are the query's own, the scores go to sim rows kstride
// apart.  CH stays the launch's: one launch per chain family present, over that family's queries, so a query runs the
// instantiation it gets alone.  PERQ == false is the kernel as it has always been.
struct RerankArgsQ : RerankArgs {
    const uint32_t* qsel;  // [gridDim.y] queries of this launch
    const int* qkind;      // [batch] by query
    const float* qcw;
    const float* qsw;
    const float* qmw;
    uint32_t kstride;
};

template <int CH, bool PERQ>
__global__ __launch_bounds__(256) void xmetric_rerank_kernel(std::conditional_t<PERQ, RerankArgsQ, RerankArgs> p) {
    __shared__ double s_mag;
    __shared__ uint32_t s_na;
    uint32_t q = blockIdx.y;
    if constexpr (PERQ) {
        q = p.qsel[blockIdx.y];
        if (blockIdx.x * kPairsPerBlock >= min(p.counts[q], p.kstride)) return;  // (the grid is as wide as the launch's longest list)
    }
    const uint32_t l = threadIdx.x & 7u, g = threadIdx.x >> 3;
    const float* a = p.queries + (size_t)q * p.dim;
    if (threadIdx.x < 8u) {  // the query's own constants: sum of squares in index order and stored positions, once
        double sa = 0.0;
        uint32_t na = 0;
        const uint32_t chunks = (p.dim + 7u) >> 3;
        for (uint32_t c = 0; c < chunks; c++) {
            const uint32_t e = 8u * c + l;
            const float x = e < p.dim ? a[e] : 0.0f;
            const bool sx = x != 0.0f;
            const double xd = sx ? (double)x : 0.0;
            na += sx ? 1u : 0u;
            sa = chain8(sa, xd * xd);
        }
        na = group8_sum(na);
        if (l == 0u) {
            s_mag = __builtin_sqrt(sa);  // magnitude_f64, sparse_vector.rs:553-559
            s_na = na;
        }
    }
    __syncthreads();
    const double mag_a = s_mag;
    const uint32_t na = s_na;
    uint32_t count, id_stride, row_len;
    int kind = p.kind;
    float cw = p.cw, sw = p.sw, mw = p.mw;
    if constexpr (PERQ) {
        count = min(p.counts[q], p.kstride);
        id_stride = row_len = p.kstride;
        kind = p.qkind[q];
        cw = p.qcw[q];
        sw = p.qsw[q];
        mw = p.qmw[q];
    } else {
        count = p.counts ? min(p.counts[q], p.c) : p.c;
        id_stride = p.id_stride;
        row_len = p.c;
    }
    const uint32_t first = blockIdx.x * kPairsPerBlock;
    const uint32_t last = min(first + kPairsPerBlock, count);
    for (uint32_t e0 = first; e0 < last; e0 += kPairsPerRound) {
        const uint32_t e = e0 + g;
        const bool used = e < last;
        const uint64_t id = used ? p.ids[(size_t)q * id_stride + e] : ~0ull;
        const bool readable = id < p.n_rows;
        const float* b = readable ? p.rows + (size_t)id * p.ld : a;  // (an unused group runs on the query: the wave stays whole)
        const PairSums s = pair_pass<CH>(a, b, p.dim, l);
        if (!used || l != 0u) continue;
        const float raw = readable ? finish_pair(kind, s, mag_a, na, cw, sw, mw) : __int_as_float(0x7FC00000);
        const size_t o = (size_t)q * row_len + e;
        if (p.raw) p.raw[o] = raw;
        if (p.sim) p.sim[o] = xm_to_similarity(kind, raw);
    }
}

// The stable descending order of each query's `count` scores (lib.rs:2611-2617): entry e goes to
// #{j : s_j > s_e} + #{j < e : s_j == s_e} — the rule hnsw_search_kernel's final ordering uses.  NaN scores (not a parity case)
// rank behind every number, among themselves by position, so the ranks are always a permutation.
struct OrderArgs {
    const float* sim;        // [nq][c]
    const uint64_t* ids;     // [nq][c]
    const uint32_t* counts;  // [nq]
    uint64_t* out_ids;       // [nq][top_k]
    float* out_scores;       // [nq][top_k]
    uint32_t* out_counts;    // [nq]
    uint32_t c, top_k;
};
__device__ __forceinline__ bool ranks_before(float sj, uint32_t j, float se, uint32_t e) {
    const bool nj = sj != sj, ne = se != se;
    if (nj || ne) return (!nj && ne) || (nj && ne && j < e);
    return sj > se || (sj == se && j < e);
}
// PERQ == true (docs/hnsw.md §12): workgroup row y orders query qsel[y] of a coalesced batch into output row y: top_k is the
// query's own (qtop[y]; 0 = this query's ordering is the large-k sort's, nothing to do here), input rows are kstride apart, output
// rows out_stride apart, and slots [min(count, top_k), out_stride) get the sentinels.  PERQ == false is the kernel as it has always been.
struct OrderArgsQ : OrderArgs {
    const uint32_t* qsel;  // [gridDim.y]
    const uint32_t* qtop;  // [gridDim.y]
    uint32_t kstride, out_stride;
};
template <bool PERQ>
__global__ __launch_bounds__(256) void xmetric_order_kernel(std::conditional_t<PERQ, OrderArgsQ, OrderArgs> p) {
    uint32_t q = blockIdx.y, o = blockIdx.y, in_stride = p.c, out_len = p.top_k, top_k = p.top_k;
    if constexpr (PERQ) {
        q = p.qsel[blockIdx.y];
        top_k = p.qtop[blockIdx.y];
        if (top_k == 0u) return;
        in_stride = p.kstride;
        out_len = p.out_stride;
    }
    const uint32_t count = min(p.counts[q], in_stride);
    const float* s = p.sim + (size_t)q * in_stride;
    const uint64_t* ids = p.ids + (size_t)q * in_stride;
    uint64_t* o_ids = p.out_ids + (size_t)o * out_len;
    float* o_sc = p.out_scores + (size_t)o * out_len;
    const uint32_t stride = gridDim.x * 256u;
    for (uint32_t e = blockIdx.x * 256u + threadIdx.x; e < count; e += stride) {
        const float se = s[e];
        uint32_t rank = 0;
        for (uint32_t j = 0; j < count; j++) rank += ranks_before(s[j], j, se, e) ? 1u : 0u;
        if (rank < top_k) {
            o_ids[rank] = ids[e];
            o_sc[rank] = se;
        }
    }
    const uint32_t n_out = min(count, top_k);
    for (uint32_t i = n_out + blockIdx.x * 256u + threadIdx.x; i < out_len; i += stride) {
        o_ids[i] = ~0ull;
        o_sc[i] = __int_as_float(0xFF800000u);
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) p.out_counts[o] = n_out;
}

constexpr uint32_t kRankMax = 16384;  // c x c comparisons a query up to here

// ---- CacheIndex::search_with_metric behind the walk (tensor_cache/src/index.rs:186-375; docs/hnsw.md §16) ---------------------------
// A candidate that is an EmbeddingStorage::Sparse node is scored on its stored entries as they are (index.rs:229-246), and a sparse
// query on its own (335-349): SparseVector's two-pointer walks (sparse_vector.rs:419-443, 816-1059), which pair the i-th duplicate
// of a position with the i-th and so differ from the dense loop above as soon as a position is stored twice.  One lane walks one
// (query, candidate) pair; the loops are lane-divergent and hold no cross-lane operation.
constexpr uint32_t kNoEntries = 0xFFFFFFFFu;  // nrec[node].z of a Dense node

// One side of a pair: an entry list in position order, or a dense row read as SparseVector::from_dense reads it (the positions with
// x != 0.0, NaN among them).
struct EntryCursor {
    const uint2* ent;
    const float* dense;
    uint32_t i, n;
    __device__ __forceinline__ void settle() {
        if (!ent)
            while (i < n && !(dense[i] != 0.0f)) i++;
    }
    __device__ __forceinline__ bool more() const { return i < n; }
    __device__ __forceinline__ uint32_t pos() const { return ent ? ent[i].x : i; }
    __device__ __forceinline__ float val() const { return ent ? __uint_as_float(ent[i].y) : dense[i]; }
    __device__ __forceinline__ void next() {
        i++;
        settle();
    }
};

// The union walk of euclidean_distance_squared_f64 / manhattan_distance / weighted_jaccard (964-1005, 1013-1052, 886-928) over a and b.
// The intersection walks of dot_f64 / jaccard_index / overlap_coefficient (419-443, 824-838, 857-871) make the same comparisons while
// both sides last and meet no equal pair afterwards, so their sums are this walk's Equal arm; magnitude_f64 (553-559) adds a side's
// squares in that side's own order, which is the order this walk consumes them in.  Every sum the chain family CH needs, in one pass.
template <int CH>
__device__ __forceinline__ PairSums merge_pass(EntryCursor a, EntryCursor b, double* sa_out, uint32_t* na_out) {
    PairSums r{0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0u, 0u};
    constexpr bool kDot = CH == kChCos || CH == kChComposite;
    constexpr bool kSd = CH == kChEucl || CH == kChComposite;
    double sa = 0.0;
    uint32_t na = 0;
    a.settle();
    b.settle();
    while (a.more() || b.more()) {
        const uint32_t pa = a.more() ? a.pos() : 0xFFFFFFFFu, pb = b.more() ? b.pos() : 0xFFFFFFFFu;  // (a position is below dim)
        const bool ta = a.more() && pa <= pb, tb = b.more() && pb <= pa;  // Less: a alone; Greater: b alone; Equal: both
        const double xd = ta ? (double)a.val() : 0.0, yd = tb ? (double)b.val() : 0.0;
        if (ta) {
            na++;
            if (kDot) sa = sa + xd * xd;
            a.next();
        }
        if (tb) {
            r.nb++;
            if (kDot) r.sb = r.sb + yd * yd;
            b.next();
        }
        if (ta && tb) {
            r.inter++;
            if (kDot) r.dot = r.dot + xd * yd;
        }
        if (kSd || CH == kChManh) {
            const double d = xd - yd;
            if (kSd) r.sd = r.sd + d * d;
            if (CH == kChManh) r.man = r.man + __builtin_fabs(d);
        }
        if (CH == kChWJ) {
            const double ax = __builtin_fabs(xd), ay = __builtin_fabs(yd);
            r.wmin = r.wmin + (ax < ay ? ax : ay);
            r.wmax = r.wmax + (ax > ay ? ax : ay);
        }
    }
    *sa_out = sa;
    *na_out = na;
    return r;
}

struct MergeArgs {
    const float* rows;       // row r at rows + r * ld
    const float* queries;    // [.][dim] (not read for a query that brings entries)
    const uint4* nrec;       // [n_rows] {entry offset lo, hi, entries or kNoEntries, .} (nullable: no Sparse node)
    const uint2* nent;       // (position, value bits) of every Sparse node
    const uint64_t* q_off;   // queries that bring entries (nullable, with q_ent and q_use)
    const uint2* q_ent;
    const uint32_t* q_use;
    const uint64_t* ids;     // [.][stride]
    const uint32_t* counts;  // [.]
    float* sim;              // [.][stride]
    // a coalesced batch (qsel non-null): workgroup row y serves query qsel[y] if qflt says it is a cache query, under its own metric
    const uint32_t* qsel;
    const uint32_t* qflt;
    const int* qkind;
    const float* qcw;
    const float* qsw;
    const float* qmw;
    uint64_t n_rows;
    uint32_t ld, dim, stride;
    int kind;
    float cw, sw, mw;
};

// sim[q][e] of every candidate that is a Sparse node, and of every candidate of a query that brings entries.  The other slots are
// xmetric_rerank_kernel's and are not touched.  An id out of bounds of such a query scores NaN, as there.
template <int CH>
__global__ __launch_bounds__(256) void xmetric_merge_kernel(MergeArgs p) {
    uint32_t q = blockIdx.y;
    int kind = p.kind;
    float cw = p.cw, sw = p.sw, mw = p.mw;
    if (p.qsel) {
        q = p.qsel[blockIdx.y];
        if (!p.qflt[q]) return;
        kind = p.qkind[q];
        cw = p.qcw[q];
        sw = p.qsw[q];
        mw = p.qmw[q];
    }
    const uint32_t count = min(p.counts[q], p.stride);
    const uint32_t e = blockIdx.x * 256u + threadIdx.x;
    if (e >= count) return;
    const size_t o = (size_t)q * p.stride + e;
    const uint64_t id = p.ids[o];
    const bool q_entries = p.q_use && p.q_use[q] != 0u;
    if (id >= p.n_rows) {
        if (q_entries) p.sim[o] = xm_to_similarity(kind, __int_as_float(0x7FC00000));
        return;
    }
    const uint4 rec = p.nrec ? p.nrec[id] : make_uint4(0u, 0u, kNoEntries, 0u);
    const bool sparse = rec.z != kNoEntries;
    if (!sparse && !q_entries) return;
    EntryCursor a, b;
    if (q_entries) {
        a.ent = p.q_ent + p.q_off[q];
        a.dense = nullptr;
        a.n = (uint32_t)(p.q_off[q + 1] - p.q_off[q]);
    } else {
        a.ent = nullptr;
        a.dense = p.queries + (size_t)q * p.dim;
        a.n = p.dim;
    }
    if (sparse) {
        b.ent = p.nent + (((uint64_t)rec.y << 32) | rec.x);
        b.dense = nullptr;
        b.n = rec.z;
    } else {
        b.ent = nullptr;
        b.dense = p.rows + (size_t)id * p.ld;
        b.n = p.dim;
    }
    a.i = b.i = 0u;
    double sa;
    uint32_t na;
    const PairSums s = merge_pass<CH>(a, b, &sa, &na);
    const float raw = finish_pair(kind, s, __builtin_sqrt(sa), na, cw, sw, mw);
    p.sim[o] = xm_to_similarity(kind, raw);
}

// The filtered ordering (index.rs:222-262): xmetric_order_kernel's rule, rank of e = #{j : s_j > s_e} + #{j < e : s_j == s_e}, over the
// PARTICIPANTS only — the entries whose id is in bounds, whose node is live (node_to_key has it, 223-226) and whose similarity
// >= threshold in f32 (248; a NaN on either side fails).  out_counts = min(participants, top_k).  At most kRankMax candidates.
struct OrderFArgs {
    const float* sim;        // [.][in_stride]
    const uint64_t* ids;     // [.][in_stride]
    const uint32_t* counts;  // [.]
    const uint32_t* live;    // one bit per node
    uint64_t* out_ids;       // [gridDim.y][out_stride]
    float* out_scores;
    uint32_t* out_counts;    // [gridDim.y]
    // a coalesced batch (qsel non-null), by output row y: the query, its top_k (0: not this kernel's) and its threshold
    const uint32_t* qsel;
    const uint32_t* qtop;
    const float* qthr;
    uint64_t n_nodes;
    uint32_t in_stride, out_stride, top_k;
    float threshold;
};
__device__ __forceinline__ bool takes_part(uint64_t id, float s, float thr, const uint32_t* __restrict__ live, uint64_t n_nodes) {
    if (id >= n_nodes) return false;
    return ((live[id >> 5] >> (uint32_t)(id & 31u)) & 1u) != 0u && s >= thr;
}
__global__ __launch_bounds__(256) void xmetric_order_filtered_kernel(OrderFArgs p) {
    __shared__ uint64_t s_part[kRankMax / 64];  // the participants of the query, one bit per entry
    uint32_t q = blockIdx.y, top_k = p.top_k;
    const uint32_t o = blockIdx.y;
    float thr = p.threshold;
    if (p.qsel) {
        q = p.qsel[o];
        top_k = p.qtop[o];
        if (top_k == 0u) return;  // (the whole workgroup)
        thr = p.qthr[o];
    }
    const uint32_t count = min(min(p.counts[q], p.in_stride), kRankMax);
    const float* s = p.sim + (size_t)q * p.in_stride;
    const uint64_t* ids = p.ids + (size_t)q * p.in_stride;
    uint64_t* o_ids = p.out_ids + (size_t)o * p.out_stride;
    float* o_sc = p.out_scores + (size_t)o * p.out_stride;
    for (uint32_t base = 0; base < count; base += 256u) {  // (uniform: every wave casts every ballot)
        const uint32_t e = base + threadIdx.x;
        const bool part = e < count && takes_part(ids[e], s[e], thr, p.live, p.n_nodes);
        const uint64_t b = __ballot(part);
        if ((threadIdx.x & 63u) == 0u) s_part[(base >> 6) + (threadIdx.x >> 6)] = b;
    }
    __syncthreads();
    const uint32_t words = ((count + 255u) >> 8) << 2;
    uint32_t n_part = 0;
    for (uint32_t w = 0; w < words; w++) n_part += (uint32_t)__popcll(s_part[w]);
    const uint32_t stride = gridDim.x * 256u;
    for (uint32_t e = blockIdx.x * 256u + threadIdx.x; e < count; e += stride) {
        if (((s_part[e >> 6] >> (e & 63u)) & 1ull) == 0ull) continue;
        const float se = s[e];
        uint32_t rank = 0;
        for (uint32_t w = 0; w < words; w++) {
            uint64_t m = s_part[w];
            while (m) {
                const uint32_t j = (w << 6) + (uint32_t)__ffsll((unsigned long long)m) - 1u;
                m &= m - 1ull;
                rank += ranks_before(s[j], j, se, e) ? 1u : 0u;
            }
        }
        if (rank < top_k) {
            o_ids[rank] = ids[e];
            o_sc[rank] = se;
        }
    }
    const uint32_t n_out = min(n_part, top_k);
    for (uint32_t i = n_out + blockIdx.x * 256u + threadIdx.x; i < p.out_stride; i += stride) {
        o_ids[i] = ~0ull;
        o_sc[i] = __int_as_float(0xFF800000u);
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) p.out_counts[o] = n_out;
}

// ---- more candidates than the rank count should order: the large-k sort (nmn_sortk.hip) --------------------------------------
// Its composite keys order by (score descending with -0.0 == +0.0, NaN last, position ascending): the same permutation as
// ranks_before, for one query per call.
uint32_t sort_from() {  // NMN_XMETRIC_SORT_FROM=<c>: the sort orders every call with more than c candidates (A/B runs, same bits);
                        // read once per call, by xmetric_order_scratch_bytes — the launcher follows what that returned
    const char* e = getenv("NMN_XMETRIC_SORT_FROM");
    return e && *e ? (uint32_t)strtoul(e, nullptr, 10) : kRankMax;
}
__global__ __launch_bounds__(256) void xmetric_sort_prep_kernel(const float* __restrict__ sim, const uint32_t* __restrict__ count_q,
                                                                uint32_t c, uint32_t* __restrict__ bits) {
    const uint32_t count = min(*count_q, c);
    for (uint32_t e = blockIdx.x * 256u + threadIdx.x; e < c; e += gridDim.x * 256u) {
        const float v = sim[e];
        bits[e] = e < count ? (v != v ? 0x7FC00000u : f2u(v)) : kScoreSentinelBits;
    }
}
// The same for the filtered ordering: an entry that does not take part is the sentinel, so the sort's own count (the keys before the
// first sentinel, reduced on the device) is the number of participants.  (A participant's score is never NaN.)
__global__ __launch_bounds__(256) void xmetric_sort_prep_filtered_kernel(const float* __restrict__ sim, const uint64_t* __restrict__ ids,
                                                                         const uint32_t* __restrict__ count_q, uint32_t c,
                                                                         const uint32_t* __restrict__ live, uint64_t n_nodes, float thr,
                                                                         uint32_t* __restrict__ bits) {
    const uint32_t count = min(*count_q, c);
    for (uint32_t e = blockIdx.x * 256u + threadIdx.x; e < c; e += gridDim.x * 256u) {
        const float v = sim[e];
        bits[e] = e < count && takes_part(ids[e], v, thr, live, n_nodes) ? f2u(v) : kScoreSentinelBits;
    }
}
__global__ __launch_bounds__(256) void xmetric_sort_gather_kernel(const uint64_t* __restrict__ pos, const float* __restrict__ sim,
                                                                  const uint64_t* __restrict__ ids, uint32_t c, uint32_t top_k,
                                                                  uint64_t* __restrict__ o_ids, float* __restrict__ o_sc) {
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < top_k; i += gridDim.x * 256u) {
        const uint64_t p = pos[i];
        const bool used = p < (uint64_t)c;
        o_ids[i] = used ? ids[p] : ~0ull;
        o_sc[i] = used ? sim[p] : __int_as_float(0xFF800000u);
    }
}
struct SortScratch {
    uint64_t* keys;
    uint64_t* pos;
    uint32_t* bits;
    float* scores;
    size_t bytes;
};
SortScratch sort_scratch(void* base, uint32_t c, uint32_t top_k) {
    SortScratch r{};
    const size_t n_keys = (size_t)largek_sort_len(c);
    r.bytes = (n_keys + top_k) * 8 + ((size_t)c + top_k) * 4;
    if (!base) return r;  // (the size alone)
    r.keys = static_cast<uint64_t*>(base);
    r.pos = r.keys + n_keys;
    r.bits = reinterpret_cast<uint32_t*>(r.pos + top_k);
    r.scores = reinterpret_cast<float*>(r.bits + c);
    return r;
}

hipError_t launch_rerank(const RerankArgs& a, hipStream_t s) {
    if (a.nq == 0 || a.c == 0) return hipSuccess;
    const dim3 grid((a.c + kPairsPerBlock - 1) / kPairsPerBlock, a.nq);
    switch (chains_of(a.kind)) {
        case kChCos: hipLaunchKernelGGL((xmetric_rerank_kernel<kChCos, false>), grid, dim3(256), 0, s, a); break;
        case kChSet: hipLaunchKernelGGL((xmetric_rerank_kernel<kChSet, false>), grid, dim3(256), 0, s, a); break;
        case kChWJ: hipLaunchKernelGGL((xmetric_rerank_kernel<kChWJ, false>), grid, dim3(256), 0, s, a); break;
        case kChEucl: hipLaunchKernelGGL((xmetric_rerank_kernel<kChEucl, false>), grid, dim3(256), 0, s, a); break;
        case kChManh: hipLaunchKernelGGL((xmetric_rerank_kernel<kChManh, false>), grid, dim3(256), 0, s, a); break;
        default: hipLaunchKernelGGL((xmetric_rerank_kernel<kChComposite, false>), grid, dim3(256), 0, s, a); break;
    }
    return hipGetLastError();
}

template <int CH>
void launch_merge_ch(const dim3& grid, hipStream_t s, const MergeArgs& a) {
    hipLaunchKernelGGL(xmetric_merge_kernel<CH>, grid, dim3(256), 0, s, a);
}
hipError_t launch_merge(int family, uint32_t c, uint32_t rows, const MergeArgs& a, hipStream_t s) {
    if (rows == 0 || c == 0) return hipSuccess;
    const dim3 grid((c + 255u) / 256u, rows);
    switch (family) {
        case kChCos: launch_merge_ch<kChCos>(grid, s, a); break;
        case kChSet: launch_merge_ch<kChSet>(grid, s, a); break;
        case kChWJ: launch_merge_ch<kChWJ>(grid, s, a); break;
        case kChEucl: launch_merge_ch<kChEucl>(grid, s, a); break;
        case kChManh: launch_merge_ch<kChManh>(grid, s, a); break;
        default: launch_merge_ch<kChComposite>(grid, s, a); break;
    }
    return hipGetLastError();
}
// the filtered ordering keeps its participants in LDS, kRankMax bits: above that the sort, whatever NMN_XMETRIC_SORT_FROM says
uint32_t sort_from_filtered(uint32_t from) { return std::min(from, kRankMax); }

}  // namespace

size_t xmetric_order_scratch_bytes(uint32_t c, uint32_t top_k, bool filtered) {
    const uint32_t from = filtered ? sort_from_filtered(sort_from()) : sort_from();
    return c > from ? sort_scratch(nullptr, c, top_k).bytes : 0;
}

bool xmetric_valid(const nmn_xmetric* m) { return m && m->kind >= NMN_XMETRIC_COSINE && m->kind <= NMN_XMETRIC_COMPOSITE; }

hipError_t launch_xmetric_rerank(const float* rows, uint32_t ld, uint32_t dim, uint64_t n_rows, const float* queries, uint32_t nq,
                                 uint32_t c, const uint64_t* cand_ids, const uint32_t* cand_counts, const nmn_xmetric& m,
                                 uint32_t top_k, float* sim, uint64_t* out_ids, float* out_scores, uint32_t* out_counts,
                                 void* order_scratch, hipStream_t s, const XmetricFilter* filter) {
    if (nq == 0) return hipSuccess;
    RerankArgs a{};
    a.rows = rows;
    a.queries = queries;
    a.ids = cand_ids;
    a.counts = cand_counts;
    a.raw = nullptr;
    a.sim = sim;
    a.n_rows = n_rows;
    a.ld = ld;
    a.dim = dim;
    a.nq = nq;
    a.c = c;
    a.id_stride = c;
    a.kind = m.kind;
    a.cw = m.cosine_weight;
    a.sw = m.structural_weight;
    a.mw = m.magnitude_weight;
    hipError_t e = launch_rerank(a, s);
    if (e != hipSuccess) return e;
    if (filter) {  // docs/hnsw.md §16: the merge re-rank over the slots that are its own, then the filtered ordering
        if (filter->nrec || filter->q_use) {
            MergeArgs g{};
            g.rows = rows;
            g.queries = queries;
            g.nrec = filter->nrec;
            g.nent = filter->nent;
            g.q_off = filter->q_off;
            g.q_ent = filter->q_ent;
            g.q_use = filter->q_use;
            g.ids = cand_ids;
            g.counts = cand_counts;
            g.sim = sim;
            g.n_rows = n_rows;
            g.ld = ld;
            g.dim = dim;
            g.stride = c;
            g.kind = m.kind;
            g.cw = m.cosine_weight;
            g.sw = m.structural_weight;
            g.mw = m.magnitude_weight;
            if ((e = launch_merge(chains_of(m.kind), c, nq, g, s)) != hipSuccess) return e;
        }
        if (order_scratch) {  // (xmetric_order_scratch_bytes(c, top_k, true) said so)
            const SortScratch w = sort_scratch(order_scratch, c, top_k);
            const uint32_t gc = std::min<uint32_t>((c + 255u) / 256u, 4096u), gk = std::min<uint32_t>((top_k + 255u) / 256u, 4096u);
            for (uint32_t q = 0; q < nq; q++) {
                const float* sim_q = sim + (size_t)q * c;
                const uint64_t* ids_q = cand_ids + (size_t)q * c;
                hipLaunchKernelGGL(xmetric_sort_prep_filtered_kernel, dim3(gc), dim3(256), 0, s, sim_q, ids_q, cand_counts + q, c,
                                   filter->live, n_rows, filter->threshold, w.bits);
                e = launch_largek(w.bits, c, w.keys, top_k, 0, w.pos, w.scores, out_counts + q, s);
                if (e != hipSuccess) return e;
                hipLaunchKernelGGL(xmetric_sort_gather_kernel, dim3(gk), dim3(256), 0, s, w.pos, sim_q, ids_q, c, top_k,
                                   out_ids + (size_t)q * top_k, out_scores + (size_t)q * top_k);
            }
            return hipGetLastError();
        }
        OrderFArgs o{};
        o.sim = sim;
        o.ids = cand_ids;
        o.counts = cand_counts;
        o.live = filter->live;
        o.out_ids = out_ids;
        o.out_scores = out_scores;
        o.out_counts = out_counts;
        o.n_nodes = n_rows;
        o.in_stride = c;
        o.out_stride = o.top_k = top_k;
        o.threshold = filter->threshold;
        const uint32_t gx = std::max<uint32_t>(1, std::min<uint32_t>((std::max(c, top_k) + 255u) / 256u, 1024u));
        hipLaunchKernelGGL(xmetric_order_filtered_kernel, dim3(gx, nq), dim3(256), 0, s, o);
        return hipGetLastError();
    }
    if (order_scratch) {  // query by query through the large-k sort (the caller's xmetric_order_scratch_bytes said so)
        const SortScratch w = sort_scratch(order_scratch, c, top_k);
        const uint32_t gc = std::min<uint32_t>((c + 255u) / 256u, 4096u), gk = std::min<uint32_t>((top_k + 255u) / 256u, 4096u);
        for (uint32_t q = 0; q < nq; q++) {
            const float* sim_q = sim + (size_t)q * c;
            hipLaunchKernelGGL(xmetric_sort_prep_kernel, dim3(gc), dim3(256), 0, s, sim_q, cand_counts + q, c, w.bits);
            e = launch_largek(w.bits, c, w.keys, top_k, 0, w.pos, w.scores, out_counts + q, s);
            if (e != hipSuccess) return e;
            hipLaunchKernelGGL(xmetric_sort_gather_kernel, dim3(gk), dim3(256), 0, s, w.pos, sim_q, cand_ids + (size_t)q * c, c, top_k,
                               out_ids + (size_t)q * top_k, out_scores + (size_t)q * top_k);
        }
        return hipGetLastError();
    }
    OrderArgs o{sim, cand_ids, cand_counts, out_ids, out_scores, out_counts, c, top_k};
    const uint32_t gx = std::max<uint32_t>(1, std::min<uint32_t>((std::max(c, top_k) + 255u) / 256u, 1024u));
    hipLaunchKernelGGL(xmetric_order_kernel<false>, dim3(gx, nq), dim3(256), 0, s, o);
    return hipGetLastError();
}

// ---- a coalesced batch: a top_k and a metric per query (docs/hnsw.md §12) ------------------------------------------------------------
// meta (u32 words, host staging and device copy alike): msel[M] | qtop[M] | fsel[M] | kind[N] | cw[N] | sw[N] | mw[N] — msel: the
// metric queries in output-row order, qtop: their top_k (0: ordered by the sort, or a cache query), fsel: the same queries grouped by
// chain family.
void xmetric_batch_plan(const XmetricBatchItem* items, uint32_t M, uint32_t N, std::vector<uint32_t>& meta, XmetricBatchPlan& plan) {
    plan = XmetricBatchPlan{};
    plan.items = items;
    plan.N = N;
    plan.M = M;
    meta.assign((size_t)5 * M + (size_t)5 * N, 0u);
    uint32_t* msel = meta.data();
    uint32_t* qtop = msel + M;
    uint32_t* fsel = qtop + M;
    uint32_t* kind = fsel + M;
    uint32_t* w[3] = {kind + N, kind + 2 * (size_t)N, kind + 3 * (size_t)N};
    // ... and behind them, for the cache queries (§16): ftop[M] | fthr[M] | qflt[N] — the filtered ordering's top_k (0: not a cache
    // query, or the sort's) and threshold by output row, and by query whether it is a cache query
    uint32_t* ftop = kind + 4 * (size_t)N;
    uint32_t* fthr = ftop + M;
    uint32_t* qflt = fthr + M;
    const uint32_t from = plan.sort_from = sort_from();  // read once per batch; the launcher follows the plan
    uint32_t fam_n[kChComposite + 1] = {};
    for (uint32_t m = 0; m < M; m++) fam_n[chains_of(items[m].m.kind)]++;
    for (int f = 0; f <= kChComposite; f++) plan.fam_off[f + 1] = plan.fam_off[f] + fam_n[f];
    uint32_t fill[kChComposite + 1];
    std::copy(plan.fam_off, plan.fam_off + kChComposite + 1, fill);
    for (uint32_t m = 0; m < M; m++) {
        const XmetricBatchItem& it = items[m];
        const int f = chains_of(it.m.kind);
        const bool sorted = it.c > (it.filter ? sort_from_filtered(from) : from);
        msel[m] = it.q;
        qtop[m] = sorted || it.filter ? 0u : it.top_k;
        if (it.filter) {
            ftop[m] = sorted ? 0u : it.top_k;
            memcpy(&fthr[m], &it.threshold, 4);
            qflt[it.q] = 1u;
            plan.fam_fc[f] = std::max(plan.fam_fc[f], it.c);
        }
        fsel[fill[f]++] = it.q;
        plan.fam_c[f] = std::max(plan.fam_c[f], it.c);
        kind[it.q] = (uint32_t)it.m.kind;
        memcpy(&w[0][it.q], &it.m.cosine_weight, 4);
        memcpy(&w[1][it.q], &it.m.structural_weight, 4);
        memcpy(&w[2][it.q], &it.m.magnitude_weight, 4);
        if (sorted)
            plan.sort_bytes = std::max(plan.sort_bytes, sort_scratch(nullptr, it.c, it.top_k).bytes);
        else if (it.filter)
            plan.frank_len = std::max(plan.frank_len, std::max(it.c, it.top_k));
        else
            plan.rank_len = std::max(plan.rank_len, std::max(it.c, it.top_k));
    }
}

hipError_t launch_xmetric_rerank_batch(const float* rows, uint32_t ld, uint32_t dim, uint64_t n_rows, const float* queries,
                                       uint32_t kstride, const uint64_t* cand_ids, const uint32_t* cand_counts,
                                       const XmetricBatchPlan& plan, const uint32_t* meta_dev, float* sim, uint32_t out_stride,
                                       uint64_t* out_ids, float* out_scores, uint32_t* out_counts, void* sort_scratch_dev,
                                       hipStream_t s, const XmetricFilter* filter) {
    const uint32_t M = plan.M, N = plan.N;
    if (M == 0) return hipSuccess;
    const uint32_t* msel = meta_dev;
    const uint32_t* qtop = msel + M;
    const uint32_t* fsel = qtop + M;
    RerankArgsQ a{};
    a.rows = rows;
    a.queries = queries;
    a.ids = cand_ids;
    a.counts = cand_counts;
    a.raw = nullptr;
    a.sim = sim;
    a.n_rows = n_rows;
    a.ld = ld;
    a.dim = dim;
    a.qkind = reinterpret_cast<const int*>(fsel + M);
    a.qcw = reinterpret_cast<const float*>(fsel + M + N);
    a.qsw = a.qcw + N;
    a.qmw = a.qsw + N;
    a.kstride = kstride;
    for (int f = 0; f <= kChComposite; f++) {  // at most one launch per chain family present, over that family's queries
        const uint32_t nf = plan.fam_off[f + 1] - plan.fam_off[f];
        if (nf == 0 || plan.fam_c[f] == 0) continue;
        a.qsel = fsel + plan.fam_off[f];
        a.nq = nf;
        const dim3 grid((plan.fam_c[f] + kPairsPerBlock - 1) / kPairsPerBlock, nf);
        switch (f) {
            case kChCos: hipLaunchKernelGGL((xmetric_rerank_kernel<kChCos, true>), grid, dim3(256), 0, s, a); break;
            case kChSet: hipLaunchKernelGGL((xmetric_rerank_kernel<kChSet, true>), grid, dim3(256), 0, s, a); break;
            case kChWJ: hipLaunchKernelGGL((xmetric_rerank_kernel<kChWJ, true>), grid, dim3(256), 0, s, a); break;
            case kChEucl: hipLaunchKernelGGL((xmetric_rerank_kernel<kChEucl, true>), grid, dim3(256), 0, s, a); break;
            case kChManh: hipLaunchKernelGGL((xmetric_rerank_kernel<kChManh, true>), grid, dim3(256), 0, s, a); break;
            default: hipLaunchKernelGGL((xmetric_rerank_kernel<kChComposite, true>), grid, dim3(256), 0, s, a); break;
        }
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    const uint32_t* ftop = fsel + M + 4 * (size_t)N;
    const float* fthr = reinterpret_cast<const float*>(ftop + M);
    const uint32_t* qflt = ftop + 2 * (size_t)M;
    if (filter && filter->nrec) {  // the cache queries' Sparse-node candidates, family by family like the dense re-rank before them
        MergeArgs g{};
        g.rows = rows;
        g.queries = queries;
        g.nrec = filter->nrec;
        g.nent = filter->nent;
        g.ids = cand_ids;
        g.counts = cand_counts;
        g.sim = sim;
        g.qflt = qflt;
        g.qkind = a.qkind;
        g.qcw = a.qcw;
        g.qsw = a.qsw;
        g.qmw = a.qmw;
        g.n_rows = n_rows;
        g.ld = ld;
        g.dim = dim;
        g.stride = kstride;
        for (int f = 0; f <= kChComposite; f++) {
            if (plan.fam_fc[f] == 0) continue;
            g.qsel = fsel + plan.fam_off[f];
            const hipError_t e = launch_merge(f, plan.fam_fc[f], plan.fam_off[f + 1] - plan.fam_off[f], g, s);
            if (e != hipSuccess) return e;
        }
    }
    if (plan.frank_len) {  // every cache query the filtered rank count orders, in one launch
        if (!filter) return hipErrorInvalidValue;
        OrderFArgs o{};
        o.sim = sim;
        o.ids = cand_ids;
        o.counts = cand_counts;
        o.live = filter->live;
        o.out_ids = out_ids;
        o.out_scores = out_scores;
        o.out_counts = out_counts;
        o.qsel = msel;
        o.qtop = ftop;
        o.qthr = fthr;
        o.n_nodes = n_rows;
        o.in_stride = kstride;
        o.out_stride = out_stride;
        const uint32_t gx = std::max<uint32_t>(1, std::min<uint32_t>((std::max(plan.frank_len, out_stride) + 255u) / 256u, 1024u));
        hipLaunchKernelGGL(xmetric_order_filtered_kernel, dim3(gx, M), dim3(256), 0, s, o);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    if (plan.rank_len) {  // every query the rank count orders, in one launch (the sorted ones' workgroups leave at once)
        OrderArgsQ o{};
        o.sim = sim;
        o.ids = cand_ids;
        o.counts = cand_counts;
        o.out_ids = out_ids;
        o.out_scores = out_scores;
        o.out_counts = out_counts;
        o.qsel = msel;
        o.qtop = qtop;
        o.kstride = kstride;
        o.out_stride = out_stride;
        const uint32_t gx = std::max<uint32_t>(1, std::min<uint32_t>((std::max(plan.rank_len, out_stride) + 255u) / 256u, 1024u));
        hipLaunchKernelGGL(xmetric_order_kernel<true>, dim3(gx, M), dim3(256), 0, s, o);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    if (plan.sort_bytes) {  // more candidates than the rank count should order: each such query alone, exactly as in a lone call
        for (uint32_t m = 0; m < M; m++) {
            const XmetricBatchItem& it = plan.items[m];
            if (it.c <= (it.filter ? sort_from_filtered(plan.sort_from) : plan.sort_from)) continue;
            const SortScratch w = sort_scratch(sort_scratch_dev, it.c, it.top_k);
            const uint32_t gc = std::min<uint32_t>((it.c + 255u) / 256u, 4096u), gk = std::min<uint32_t>((it.top_k + 255u) / 256u, 4096u);
            const float* sim_q = sim + (size_t)it.q * kstride;
            if (it.filter) {
                if (!filter) return hipErrorInvalidValue;
                hipLaunchKernelGGL(xmetric_sort_prep_filtered_kernel, dim3(gc), dim3(256), 0, s, sim_q, cand_ids + (size_t)it.q * kstride,
                                   cand_counts + it.q, it.c, filter->live, n_rows, it.threshold, w.bits);
            } else
                hipLaunchKernelGGL(xmetric_sort_prep_kernel, dim3(gc), dim3(256), 0, s, sim_q, cand_counts + it.q, it.c, w.bits);
            const hipError_t e = launch_largek(w.bits, it.c, w.keys, it.top_k, 0, w.pos, w.scores, out_counts + m, s);
            if (e != hipSuccess) return e;
            hipLaunchKernelGGL(xmetric_sort_gather_kernel, dim3(gk), dim3(256), 0, s, w.pos, sim_q, cand_ids + (size_t)it.q * kstride, it.c,
                               it.top_k, out_ids + (size_t)m * out_stride, out_scores + (size_t)m * out_stride);
        }
        return hipGetLastError();
    }
    return hipSuccess;
}

}  // namespace nmn

using namespace nmn;

// ---- the C ABI -------------------------------------------------------------------------------------------------------------
static void set_geometric(nmn_xmetric* m, float cw, float sw, float mw) {
    if (!m) return;
    m->kind = NMN_XMETRIC_COMPOSITE;
    m->cosine_weight = cw;
    m->structural_weight = sw;
    m->magnitude_weight = mw;
}
extern "C" void nmn_xmetric_geometric_default(nmn_xmetric* m) { set_geometric(m, 0.5f, 0.3f, 0.2f); }             // distance.rs:127-135
extern "C" void nmn_xmetric_geometric_angular_heavy(nmn_xmetric* m) { set_geometric(m, 0.8f, 0.1f, 0.1f); }       // 140-146
extern "C" void nmn_xmetric_geometric_structural_heavy(nmn_xmetric* m) { set_geometric(m, 0.2f, 0.7f, 0.1f); }    // 150-156
extern "C" void nmn_xmetric_geometric_conflict_detection(nmn_xmetric* m) { set_geometric(m, 0.4f, 0.5f, 0.1f); }  // 160-166

extern "C" float nmn_xmetric_to_similarity(const nmn_xmetric* m, float raw) {
    if (!xmetric_valid(m)) return std::nanf("");
    return xm_to_similarity(m->kind, raw);
}

extern "C" int32_t nmn_xmetric_higher_is_better(const nmn_xmetric* m) {  // distance.rs:60-69
    if (!xmetric_valid(m)) return 0;
    switch (m->kind) {
        case NMN_XMETRIC_COSINE:
        case NMN_XMETRIC_JACCARD:
        case NMN_XMETRIC_OVERLAP:
        case NMN_XMETRIC_WEIGHTED_JACCARD:
        case NMN_XMETRIC_COMPOSITE: return 1;
        default: return 0;
    }
}

extern "C" nmn_status nmn_index_score_rows_xmetric(nmn_index* idx, const float* queries, uint32_t nq, const nmn_xmetric* metric,
                                                   const uint64_t* local_rows, uint32_t n_rows, float* out_raw,
                                                   float* out_similarity) {
    if (!idx || !queries || !local_rows || !metric) return set_error(NMN_ERR_INVALID_ARGUMENT, "null argument");
    if (!xmetric_valid(metric)) return set_error(NMN_ERR_CONFIGURATION, "unknown extended distance metric");
    if (nq == 0 || n_rows == 0 || (!out_raw && !out_similarity)) return NMN_OK;
    if (nq > NMN_MAX_QUERIES) return set_error(NMN_ERR_INVALID_ARGUMENT, "nq out of range");
    hipError_t e = hipSetDevice(idx->device);
    if (e != hipSuccess) return set_error_hip(e, "hipSetDevice");
    // idx->mu for the whole call, without nmn_index_score_rows' wait for idle slots: this only READS the rows, into buffers of its
    // own, on host_stream behind every upload; searches in flight on the other slots read too.  Writers take idx->mu, so none runs
    // under it.
    std::unique_lock<std::mutex> lk(idx->mu);
    for (uint32_t i = 0; i < n_rows; i++)
        if (local_rows[i] >= idx->rows) return set_error(NMN_ERR_NOT_FOUND, "row out of range");
    hipStream_t s = idx->host_stream;
    const size_t n_out = (size_t)nq * n_rows;
    float *dq = nullptr, *draw = nullptr, *dsim = nullptr;
    uint64_t* drows = nullptr;
    auto done = [&](nmn_status st) {
        for (void* p : {(void*)dq, (void*)draw, (void*)dsim, (void*)drows})
            if (p) (void)hipFree(p);
        return st;
    };
#define XM_TRY(x) if ((e = (x)) != hipSuccess) return done(set_error_hip(e, #x))
    XM_TRY(hipMalloc(reinterpret_cast<void**>(&dq), (size_t)nq * idx->dim * 4));
    XM_TRY(hipMalloc(reinterpret_cast<void**>(&draw), n_out * 4));
    XM_TRY(hipMalloc(reinterpret_cast<void**>(&dsim), n_out * 4));
    XM_TRY(hipMalloc(reinterpret_cast<void**>(&drows), (size_t)n_rows * 8));
    XM_TRY(hipMemcpyAsync(dq, queries, (size_t)nq * idx->dim * 4, hipMemcpyHostToDevice, s));
    XM_TRY(hipMemcpyAsync(drows, local_rows, (size_t)n_rows * 8, hipMemcpyHostToDevice, s));
    RerankArgs a{};
    a.rows = idx->corpus;
    a.queries = dq;
    a.ids = drows;
    a.counts = nullptr;
    a.raw = draw;
    a.sim = dsim;
    a.n_rows = idx->rows;
    a.ld = idx->ld;
    a.dim = idx->dim;
    a.nq = nq;
    a.c = n_rows;
    a.id_stride = 0;
    a.kind = metric->kind;
    a.cw = metric->cosine_weight;
    a.sw = metric->structural_weight;
    a.mw = metric->magnitude_weight;
    XM_TRY(launch_rerank(a, s));
    if (out_raw) XM_TRY(hipMemcpyAsync(out_raw, draw, n_out * 4, hipMemcpyDeviceToHost, s));
    if (out_similarity) XM_TRY(hipMemcpyAsync(out_similarity, dsim, n_out * 4, hipMemcpyDeviceToHost, s));
    XM_TRY(hipStreamSynchronize(s));
#undef XM_TRY
    return done(NMN_OK);
}

extern "C" nmn_status nmn_xmetric_score_host_rows(int32_t device, const float* rows_host, uint32_t n_rows, uint32_t dim,
                                                  const float* query, const nmn_xmetric* metric, float* out_raw,
                                                  float* out_similarity) {
    if (!rows_host || !query || !metric) return set_error(NMN_ERR_INVALID_ARGUMENT, "null argument");
    if (!xmetric_valid(metric)) return set_error(NMN_ERR_CONFIGURATION, "unknown extended distance metric");
    if (dim == 0) return set_error(NMN_ERR_EMPTY_VECTOR, "dim == 0");
    if (n_rows == 0 || (!out_raw && !out_similarity)) return NMN_OK;
    hipError_t e;
    if (device >= 0 && (e = hipSetDevice(device)) != hipSuccess) return set_error_hip(e, "hipSetDevice");
    // one block for the call: rows | query | ids 0 .. n-1 | raw | similarity
    const size_t row_bytes = (size_t)n_rows * dim * 4, q_bytes = ((size_t)dim * 4 + 7) & ~(size_t)7;
    const size_t ids_off = ((row_bytes + 7) & ~(size_t)7) + q_bytes, raw_off = ids_off + (size_t)n_rows * 8;
    std::vector<uint64_t> ids(n_rows);
    for (uint32_t i = 0; i < n_rows; i++) ids[i] = i;
    uint8_t* blk = nullptr;
    if ((e = hipMalloc(reinterpret_cast<void**>(&blk), raw_off + (size_t)n_rows * 8)) != hipSuccess) return set_error_hip(e, "hipMalloc");
    auto done = [&](nmn_status st) {
        (void)hipFree(blk);
        return st;
    };
    hipStream_t s = hipStreamPerThread;
    float* d_rows = reinterpret_cast<float*>(blk);
    float* d_q = reinterpret_cast<float*>(blk + ids_off - q_bytes);
    float* d_raw = reinterpret_cast<float*>(blk + raw_off);
#define XM_TRY(x) if ((e = (x)) != hipSuccess) return done(set_error_hip(e, #x))
    XM_TRY(hipMemcpyAsync(d_rows, rows_host, row_bytes, hipMemcpyHostToDevice, s));
    XM_TRY(hipMemcpyAsync(d_q, query, (size_t)dim * 4, hipMemcpyHostToDevice, s));
    XM_TRY(hipMemcpyAsync(blk + ids_off, ids.data(), (size_t)n_rows * 8, hipMemcpyHostToDevice, s));
    RerankArgs a{};
    a.rows = d_rows;
    a.queries = d_q;
    a.ids = reinterpret_cast<const uint64_t*>(blk + ids_off);
    a.counts = nullptr;
    a.raw = d_raw;
    a.sim = d_raw + n_rows;
    a.n_rows = n_rows;
    a.ld = dim;
    a.dim = dim;
    a.nq = 1;
    a.c = n_rows;
    a.id_stride = 0;
    a.kind = metric->kind;
    a.cw = metric->cosine_weight;
    a.sw = metric->structural_weight;
    a.mw = metric->magnitude_weight;
    XM_TRY(launch_rerank(a, s));
    if (out_raw) XM_TRY(hipMemcpyAsync(out_raw, a.raw, (size_t)n_rows * 4, hipMemcpyDeviceToHost, s));
    if (out_similarity) XM_TRY(hipMemcpyAsync(out_similarity, a.sim, (size_t)n_rows * 4, hipMemcpyDeviceToHost, s));
    XM_TRY(hipStreamSynchronize(s));
#undef XM_TRY
    return done(NMN_OK);
}
