// nmn_sparse_canon.hip — SparseVector::try_from_parts (sparse_vector.rs:155-193), magnitude (548-559) and to_dense (400-406) of a
// CSR of queries that sits in DEVICE memory: what canonicalise_sparse (nmn_hnsw_build.hip) and SparseQueries::to_dense do on the
// host, bit for bit, in front of nmn_hnsw_search_sparse_device / nmn_hnsw_cache_search_sparse_device (docs/hnsw.md §22).
// THIS TRANSLATION UNIT IS BUILT WITH -ffp-contract=off -fhip-fp32-correctly-rounded-divide-sqrt (build.py): the magnitude is the
// reference's f64 chain and must give its bits.
//
// Three launches on the caller's stream, nothing read back:
//   sparse_count_kernel   one workgroup per query: the status (2: the range, 1: a position >= dim, 3: a duplicated position where the
//                         caller refuses them) and the kept count — the raw entries with val != 0.0 — into off[q + 1]
//   sparse_scan_kernel    one wave: off[] becomes the running sum of the counts, 64 at a time with a carry
//   sparse_sort_kernel    one workgroup per query: the bitonic sort of the keys (position << 32 | input index) in LDS, the packed
//                         (position, value bits) pairs at off[q], the duplicate flag, the to_dense() row, and the magnitude
#include "nmn_hnsw_handle.h"

#pragma clang fp contract(off)

using namespace nmn;
using namespace nmn::hnsw;

namespace {

constexpr uint32_t kCanonThreads = 256;
constexpr uint32_t kCanonGridMax = 1024;  // workgroups of one launch; the queries beyond are taken in a grid-stride loop
constexpr uint64_t kPadKey = ~0ull;       // a dropped entry, and a slot past the raw count: sorts behind every kept key

struct CanonArgs {
    const uint64_t* indptr;  // [nq + 1]
    const uint32_t* pos;     // [nnz_total]
    const float* val;        // [nnz_total]
    uint64_t nnz_total;
    uint32_t nq, dim, max_nnz;  // max_nnz <= kSparseLdsEntries
    uint32_t refuse_dup;        // != 0: a query with a duplicated position among its kept entries gets status 3
    uint64_t* off;              // [nq + 1]
    uint2* ent;                 // [nnz_total]
    float* mag;                 // [nq]
    uint32_t* dup;              // [nq] nullable
    float* dense;               // [nq][dim] nullable
    uint32_t* status;           // [nq]
};

// The raw range of query q, checked against everything a read of it depends on.  false: status 2.
__device__ __forceinline__ bool raw_range(const CanonArgs& a, uint32_t q, uint64_t* lo, uint32_t* n) {
    const uint64_t b = a.indptr[q], e = a.indptr[q + 1];
    if (e < b || e > a.nnz_total || e - b > a.max_nnz) return false;
    *lo = b;
    *n = (uint32_t)(e - b);
    return true;
}

__global__ __launch_bounds__(kCanonThreads) void sparse_count_kernel(CanonArgs a) {
    __shared__ uint32_t seen[kMaxDim / 32];  // one bit per position (refuse_dup only)
    __shared__ uint32_t s_bad, s_kept, s_dup;
    const uint32_t tid = threadIdx.x;
    for (uint32_t q = blockIdx.x; q < a.nq; q += gridDim.x) {
        uint64_t lo = 0;
        uint32_t n = 0, st = 2u, kept = 0;
        if (raw_range(a, q, &lo, &n)) {  // (the same for every thread of the workgroup)
            if (tid == 0) s_bad = s_kept = s_dup = 0u;
            if (a.refuse_dup)
                for (uint32_t w = tid; w < kMaxDim / 32; w += kCanonThreads) seen[w] = 0u;
            __syncthreads();
            uint32_t bad = 0, mine = 0, twice = 0;
            for (uint32_t i = tid; i < n; i += kCanonThreads) {
                const uint32_t p = a.pos[lo + i];
                if (p >= a.dim) {  // before the value is looked at: IndexOutOfBounds comes first on the host too
                    bad = 1u;
                    continue;
                }
                if (a.val[lo + i] != 0.0f) {
                    mine++;
                    if (a.refuse_dup && ((atomicOr(&seen[p >> 5], 1u << (p & 31u)) >> (p & 31u)) & 1u) != 0u) twice = 1u;
                }
            }
            if (bad) atomicOr(&s_bad, 1u);
            if (twice) atomicOr(&s_dup, 1u);
            if (mine) atomicAdd(&s_kept, mine);
            __syncthreads();
            st = s_bad ? 1u : s_dup ? 3u : 0u;
            kept = st ? 0u : s_kept;
            __syncthreads();  // (the next query resets the three words)
        }
        if (tid == 0) {
            a.status[q] = st;
            a.off[q + 1] = kept;
        }
    }
}

// off[q + 1] = count of query q on entry, the sum of the counts of queries 0 .. q on exit; off[0] = 0.  `cap` is the entries the
// packed array holds: the counts of a well-formed CSR never pass it (its ranges are disjoint), and a query that would — possible
// only where indptr decreases somewhere, so that two ranges overlap — gets status 2 and the count 0 instead of a write out of bounds.
__global__ __launch_bounds__(64) void sparse_scan_kernel(uint64_t* off, uint32_t* status, uint32_t nq, uint64_t cap) {
    const uint32_t lane = threadIdx.x;
    uint64_t carry = 0;
    if (lane == 0) off[0] = 0;
    for (uint32_t q0 = 0; q0 < nq; q0 += 64u) {
        const uint32_t q = q0 + lane;
        unsigned long long c = q < nq ? off[q + 1] : 0ull;
        unsigned long long incl;
        for (;;) {
            incl = c;
            for (uint32_t d = 1; d < 64u; d <<= 1) {
                const unsigned long long t = __shfl_up(incl, d);
                if (lane >= d) incl += t;
            }
            const unsigned long long over = __ballot(carry + incl > cap);
            if (!over) break;
            if (lane == (uint32_t)__ffsll(over) - 1u) {  // the first that does not fit (its count is not 0: the lanes before it fit)
                c = 0;
                status[q] = 2u;
            }
        }
        if (q < nq) off[q + 1] = carry + incl;
        carry += __shfl(incl, 63);
    }
}

// Dynamic LDS: P keys of 8 bytes, then P values of 4, P = max_nnz rounded up to a power of two (48 KiB at 4096).
__global__ __launch_bounds__(kCanonThreads) void sparse_sort_kernel(CanonArgs a, uint32_t pmax) {
    extern __shared__ __attribute__((aligned(8))) unsigned char canon_lds[];
    uint64_t* keys = reinterpret_cast<uint64_t*>(canon_lds);
    float* sval = reinterpret_cast<float*>(canon_lds + (size_t)pmax * 8);
    __shared__ uint32_t s_dup;
    const uint32_t tid = threadIdx.x;
    for (uint32_t q = blockIdx.x; q < a.nq; q += gridDim.x) {
        uint64_t lo = 0;
        uint32_t n = 0, kept = 0;
        const uint64_t o0 = a.off[q], o1 = a.off[q + 1];
        if (a.status[q] == 0u && raw_range(a, q, &lo, &n) && o1 >= o0 && o1 <= a.nnz_total)
            kept = (uint32_t)min((uint64_t)n, o1 - o0);  // (what the scan gave this query room for)
        else
            n = 0;  // every other query is the entry-less one
        uint32_t p2 = 1;
        while (p2 < n) p2 <<= 1;
        if (tid == 0) s_dup = 0u;
        for (uint32_t i = tid; i < p2; i += kCanonThreads) {
            uint64_t key = kPadKey;
            if (i < n) {
                const uint32_t p = a.pos[lo + i];
                if (p < a.dim && a.val[lo + i] != 0.0f) key = ((uint64_t)p << 32) | i;
            }
            keys[i] = key;
        }
        __syncthreads();
        // the keys are unique, so the network's order is the stable order by position
        for (uint32_t k = 2; k <= p2; k <<= 1) {
            for (uint32_t j = k >> 1; j > 0; j >>= 1) {
                for (uint32_t i = tid; i < p2; i += kCanonThreads) {
                    const uint32_t x = i ^ j;
                    if (x > i) {
                        const uint64_t u = keys[i], v = keys[x];
                        if ((u > v) == ((i & k) == 0u)) {
                            keys[i] = v;
                            keys[x] = u;
                        }
                    }
                }
                __syncthreads();
            }
        }
        // the packed entries, the values in canonical order into LDS, the duplicate flag
        uint32_t twice = 0;
        for (uint32_t i = tid; i < kept; i += kCanonThreads) {
            const uint64_t key = keys[i];
            const bool ok = key != kPadKey;  // (false only if the arrays changed under the call)
            const uint32_t p = ok ? (uint32_t)(key >> 32) : 0u;
            const float v = ok ? a.val[lo + (uint32_t)key] : 0.0f;
            sval[i] = v;
            a.ent[o0 + i] = make_uint2(p, __float_as_uint(v));
            if (i > 0 && ok && (uint32_t)(keys[i - 1] >> 32) == p) twice = 1u;
        }
        if (twice) atomicOr(&s_dup, 1u);
        __syncthreads();
        if (a.dense) {  // zeros, then the entries in order: the last entry of a run of equal positions wins
            float* row = a.dense + (size_t)q * a.dim;
            for (uint32_t d = tid; d < a.dim; d += kCanonThreads) {
                uint32_t b = 0, e = kept;  // the first entry whose position is above d
                while (b < e) {
                    const uint32_t mid = (b + e) >> 1;
                    if ((uint32_t)(keys[mid] >> 32) <= d)
                        b = mid + 1;
                    else
                        e = mid;
                }
                row[d] = b > 0 && (uint32_t)(keys[b - 1] >> 32) == d ? sval[b - 1] : 0.0f;
            }
        }
        if (tid == 0 && a.dup) a.dup[q] = s_dup;
        __syncthreads();
        // magnitude(): the products are exact in f64 and independent, every thread forms its own over the keys' slots; the sum is
        // ONE chain from -0.0 in canonical order, one rounding per add, so a single lane runs it
        for (uint32_t i = tid; i < kept; i += kCanonThreads) {
            const double v = (double)sval[i];
            keys[i] = (uint64_t)__double_as_longlong(v * v);
        }
        __syncthreads();
        if (tid == 0) {
            double acc = -0.0;
            for (uint32_t i = 0; i < kept; i++) acc = acc + __longlong_as_double((long long)keys[i]);
            a.mag[q] = (float)__builtin_sqrt(acc);
        }
        __syncthreads();  // (the next query overwrites the keys)
    }
}

// The rows of the queries a search entry did not serve: count 0, ids UINT64_MAX, scores -inf.
__global__ __launch_bounds__(kCanonThreads) void sparse_status_rows_kernel(const uint32_t* status, uint32_t nq, uint32_t k, uint64_t* ids,
                                                                           float* scores, uint32_t* counts) {
    const uint32_t q = blockIdx.x * kCanonThreads + threadIdx.x;
    if (q >= nq || status[q] == 0u) return;
    counts[q] = 0u;
    for (uint32_t i = 0; i < k; i++) {
        ids[(size_t)q * k + i] = ~0ull;
        scores[(size_t)q * k + i] = -INFINITY;
    }
}

}  // namespace

namespace nmn {
namespace hnsw {

nmn_status launch_sparse_canon(uint32_t dim, const uint64_t* indptr_dev, const uint32_t* positions_dev, const float* values_dev,
                               uint32_t nq, uint64_t nnz_total, uint32_t max_nnz, bool refuse_dup, uint64_t* off_dev, uint32_t* entries_dev,
                               float* mag_dev, uint32_t* dup_dev, float* dense_dev, uint32_t* status_dev, hipStream_t s) {
    CanonArgs a{};
    a.indptr = indptr_dev;
    a.pos = positions_dev;
    a.val = values_dev;
    a.nnz_total = nnz_total;
    a.nq = nq;
    a.dim = dim;
    a.max_nnz = max_nnz;
    a.refuse_dup = refuse_dup ? 1u : 0u;
    a.off = off_dev;
    a.ent = reinterpret_cast<uint2*>(entries_dev);
    a.mag = mag_dev;
    a.dup = dup_dev;
    a.dense = dense_dev;
    a.status = status_dev;
    uint32_t pmax = 1;
    while (pmax < max_nnz) pmax <<= 1;
    const uint32_t grid = std::min(nq, kCanonGridMax);
    sparse_count_kernel<<<grid, kCanonThreads, 0, s>>>(a);
    HN_TRY(hipGetLastError());
    sparse_scan_kernel<<<1, 64, 0, s>>>(off_dev, status_dev, nq, nnz_total);
    HN_TRY(hipGetLastError());
    sparse_sort_kernel<<<grid, kCanonThreads, (size_t)pmax * 12, s>>>(a, pmax);
    HN_TRY(hipGetLastError());
    return NMN_OK;
}

nmn_status launch_sparse_status_rows(const uint32_t* status_dev, uint32_t nq, uint32_t k, uint64_t* ids_dev, float* scores_dev,
                                     uint32_t* counts_dev, hipStream_t s) {
    sparse_status_rows_kernel<<<(nq + kCanonThreads - 1) / kCanonThreads, kCanonThreads, 0, s>>>(status_dev, nq, k, ids_dev, scores_dev,
                                                                                                  counts_dev);
    HN_TRY(hipGetLastError());
    return NMN_OK;
}

nmn_status sparse_max_nnz(uint32_t dim, uint32_t max_nnz, uint32_t* out) {
    if (max_nnz > kSparseLdsEntries)
        return set_error(NMN_ERR_INVALID_ARGUMENT, "sparse queries: max_nnz above 4096, the raw entries of one query a workgroup sorts in LDS");
    *out = max_nnz ? max_nnz : std::min(dim, kSparseLdsEntries);
    return NMN_OK;
}

}  // namespace hnsw
}  // namespace nmn

extern "C" nmn_status nmn_sparse_canonicalise_device(uint32_t dim, const uint64_t* indptr_dev, const uint32_t* positions_dev,
                                                     const float* values_dev, uint32_t nq, uint64_t nnz_total, uint32_t max_nnz,
                                                     uint64_t* out_off_dev, uint32_t* out_entries_dev, float* out_mag_dev,
                                                     uint32_t* out_dup_dev, float* out_dense_dev, uint32_t* out_status_dev, int32_t device,
                                                     void* stream) {
    uint32_t mx = 0;
    if (const nmn_status sm = sparse_max_nnz(dim, max_nnz, &mx); sm != NMN_OK) return sm;
    if (dim == 0) return set_error(NMN_ERR_EMPTY_VECTOR, "dim == 0");
    if (dim > kMaxDim) return set_error(NMN_ERR_CONFIGURATION, "sparse queries: dimension above 8192");
    if (nq == 0) return NMN_OK;
    if (!indptr_dev || !out_off_dev || !out_entries_dev || !out_mag_dev || !out_status_dev || (nnz_total && (!positions_dev || !values_dev)))
        return set_error(NMN_ERR_INVALID_ARGUMENT, "null argument");
    if (device >= 0) HN_TRY(hipSetDevice(device));
    return launch_sparse_canon(dim, indptr_dev, positions_dev, values_dev, nq, nnz_total, mx, false, out_off_dev, out_entries_dev,
                               out_mag_dev, out_dup_dev, out_dense_dev, out_status_dev, static_cast<hipStream_t>(stream));
}
