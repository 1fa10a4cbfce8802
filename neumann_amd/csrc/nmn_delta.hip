// nmn_delta.hip — DeltaVector and ArchetypeRegistry (tensor_store/src/delta_vector.rs:72-643) on the GPU, bit for bit: the registry
// handle nmn_archetypes, the set handle nmn_delta_set, their kernels and the host restatement of the same chains (docs/delta.md).
// Built with -ffp-contract=off -fhip-fp32-correctly-rounded-divide-sqrt like nmn_exact.hip: every sum below is a strictly sequential
// f32 chain in the reference's order, products rounded before they are added.  The summation order forbids MFMA and any split of a
// chain over lanes, so the parallelism is across chains only: rows x archetypes, rows, (query, row) pairs.
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstring>
#include <functional>
#include <mutex>
#include <shared_mutex>
#include <string>
#include <thread>
#include <vector>

#include "nmn_internal.h"
#include "nmn_select_dev.h"

#pragma clang fp contract(off)

using namespace nmn;

namespace {

constexpr uint32_t kArchTile = 8;      // archetypes whose chains one lane of find_best carries in registers
constexpr uint32_t kDimChunk = 64;     // dimensions staged through LDS per step of find_best
constexpr uint32_t kScanBlock = 256;   // rows per step of the single-workgroup offset scan
constexpr uint32_t kLdsQueryDim = 8192;  // a query up to this dimension sits in LDS (32 KiB) while a slice is scored
constexpr uint32_t kQueryBlock = 32768;  // queries per launch of the score kernels (gridDim.y is 16 bits wide)
constexpr uint64_t kChunkBytes = 256ull << 20;  // dense rows on the device per step of a host-buffer call
constexpr uint32_t kSelectMaxK = 4096;                // the largest k deltaset_select_kernel serves: its composites fill 32 KiB of LDS
constexpr uint32_t kSelectChunk = kSelThreads * 4;    // score words one step of its workgroup reads: 16 bytes per lane
constexpr uint64_t kSearchBudget = 256ull << 20;      // score words [queries][n] on the device per step of a host-buffer search
constexpr uint64_t kSortSingleRows = 1ull << 18;      // a single query over this many rows is ranked by the sort, not by one workgroup

#define HD __host__ __device__ inline

// ---- the chains, one implementation for the kernels and the host ------------------------------------------------------------
// `.map(|x| x * x).sum::<f32>()`: folds from -0.0
HD float chain_sq(const float* x, uint64_t n) {
    float s = -0.0f;
    for (uint64_t i = 0; i < n; i++) {
        const float p = x[i] * x[i];
        s = s + p;
    }
    return s;
}
// `.zip().map(|(a, b)| a * b).sum::<f32>()`
HD float chain_dot(const float* a, const float* b, uint64_t n) {
    float s = -0.0f;
    for (uint64_t i = 0; i < n; i++) {
        const float p = a[i] * b[i];
        s = s + p;
    }
    return s;
}
// find_best_archetype's similarity of one archetype (499-504)
HD float arch_sim(float dot, float magnitude_sq, float query_mag) {
    const float arch_mag = sqrtf(magnitude_sq);
    if (arch_mag == 0.0f) return 0.0f;
    const float den = arch_mag * query_mag;
    return dot / den;
}
// `delta.abs() > threshold` (133-134): false for a NaN on either side
HD bool delta_kept(float val, float ref, float threshold, float* delta) {
    *delta = val - ref;
    return fabsf(*delta) > threshold;
}
// dot_dense_with_precomputed's delta_dot (297-302): entry e of the row sits at [e * stride]; never touches an entry past `len`
HD float gather_dot(const uint16_t* pos, const float* del, uint64_t len, uint64_t stride, const float* query) {
    float s = -0.0f;
    for (uint64_t e = 0; e < len; e++) {
        const float p = del[e * stride] * query[pos[e * stride]];
        s = s + p;
    }
    return s;
}
// cosine_similarity_dense (374-388) after the dot
HD float cosine_of(float dot, float self_magnitude, float query_magnitude) {
    if (self_magnitude == 0.0f || query_magnitude == 0.0f) return 0.0f;
    const float den = self_magnitude * query_magnitude;
    return dot / den;
}
// dot_same_archetype (321-349) with sparse_delta_dot (352-370), the merge loop as written
HD float pair_dot(const uint16_t* pa, const float* da, uint64_t na, const uint16_t* pb, const float* db, uint64_t nb,
                  const float* archetype, float magnitude_sq) {
    float r_dot_delta_b = -0.0f;
    for (uint64_t e = 0; e < nb; e++) {
        const float p = archetype[pb[e]] * db[e];
        r_dot_delta_b = r_dot_delta_b + p;
    }
    float delta_a_dot_r = -0.0f;
    for (uint64_t e = 0; e < na; e++) {
        const float p = da[e] * archetype[pa[e]];
        delta_a_dot_r = delta_a_dot_r + p;
    }
    float result = 0.0f;  // `let mut result = 0.0`
    uint64_t i = 0, j = 0;
    while (i < na && j < nb) {
        if (pa[i] < pb[j]) {
            i++;
        } else if (pa[i] > pb[j]) {
            j++;
        } else {
            const float p = da[i] * db[j];
            result = result + p;
            i++;
            j++;
        }
    }
    float s = magnitude_sq + r_dot_delta_b;
    s = s + delta_a_dot_r;
    return s + result;
}
// to_dense (209-217) into `out`, which already holds the archetype
HD void apply_deltas(const uint16_t* pos, const float* del, uint64_t len, float* out) {
    for (uint64_t e = 0; e < len; e++) out[pos[e]] = out[pos[e]] + del[e];
}

// ---- kernels ----------------------------------------------------------------------------------------------------------------

// find_best_archetype for 64 rows per workgroup (one wave): a lane owns one row and the running chains of kArchTile archetypes; the
// rows' and the archetypes' next kDimChunk dimensions are staged through LDS (coalesced loads; xs is read down its padded columns
// without bank conflicts, as_ as a broadcast).  Tiles come in ascending id order and a candidate wins only under `>`.
// mags_out (nullable) gets query_mag, the cached magnitude of from_dense_with_reference_and_magnitude.
__global__ void __launch_bounds__(64) delta_find_best_kernel(const float* __restrict__ rows, uint64_t n, uint32_t dim,
                                                             const float* __restrict__ arch, const float* __restrict__ msq, uint32_t K,
                                                             int64_t* __restrict__ ids_out, float* __restrict__ sims_out,
                                                             float* __restrict__ mags_out) {
    __shared__ float xs[64][kDimChunk + 1];
    __shared__ float as_[kArchTile][kDimChunk];
    const uint32_t lane = threadIdx.x;
    const uint64_t row0 = (uint64_t)blockIdx.x * 64;
    const uint32_t nrows = (uint32_t)(n - row0 < 64 ? n - row0 : 64);
    const bool active = lane < nrows;
    float qsum = -0.0f, query_mag = 0.0f;
    float best_sim = -INFINITY;
    uint32_t best_id = 0;
    const uint32_t ntiles = K ? (K + kArchTile - 1) / kArchTile : 1;  // K == 0: the magnitude alone
    for (uint32_t tile = 0; tile < ntiles; tile++) {
        const uint32_t a0 = tile * kArchTile;
        const uint32_t tc = K - a0 < kArchTile ? K - a0 : kArchTile;
        float acc[kArchTile];
#pragma unroll
        for (uint32_t t = 0; t < kArchTile; t++) acc[t] = -0.0f;
        for (uint32_t d0 = 0; d0 < dim; d0 += kDimChunk) {
            const uint32_t cw = dim - d0 < kDimChunk ? dim - d0 : kDimChunk;
            __syncthreads();
            if (lane < cw) {
                for (uint32_t r = 0; r < nrows; r++) xs[r][lane] = rows[(row0 + r) * dim + d0 + lane];
                for (uint32_t t = 0; t < tc; t++) as_[t][lane] = arch[(uint64_t)(a0 + t) * dim + d0 + lane];
            }
            __syncthreads();
            if (active) {
                for (uint32_t d = 0; d < cw; d++) {
                    const float x = xs[lane][d];
                    if (tile == 0) {
                        const float p = x * x;
                        qsum = qsum + p;
                    }
#pragma unroll
                    for (uint32_t t = 0; t < kArchTile; t++) {
                        if (t < tc) {
                            const float p = as_[t][d] * x;
                            acc[t] = acc[t] + p;
                        }
                    }
                }
            }
        }
        if (tile == 0) query_mag = sqrtf(qsum);
        if (active) {
#pragma unroll
            for (uint32_t t = 0; t < kArchTile; t++) {
                if (t < tc) {
                    const float sim = arch_sim(acc[t], msq[a0 + t], query_mag);
                    if (sim > best_sim) {
                        best_sim = sim;
                        best_id = a0 + t;
                    }
                }
            }
        }
    }
    if (!active) return;
    if (query_mag == 0.0f) {  // `return Some((0, 0.0))`
        best_id = 0;
        best_sim = 0.0f;
    }
    const uint64_t row = row0 + lane;
    if (ids_out) ids_out[row] = (int64_t)best_id;
    if (sims_out) sims_out[row] = best_sim;
    if (mags_out) mags_out[row] = query_mag;
}

// try_from_dense_with_reference, pass 1: a wave per row counts the kept positions, 64 per step.
__global__ void __launch_bounds__(256) delta_count_kernel(const float* __restrict__ rows, uint64_t n, uint32_t dim,
                                                          const float* __restrict__ arch, const int64_t* __restrict__ ids, float threshold,
                                                          uint32_t* __restrict__ counts) {
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t row = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= n) return;  // a whole wave leaves together
    const float* x = rows + row * dim;
    const float* a = arch + (uint64_t)ids[row] * dim;
    uint32_t count = 0;
    for (uint32_t base = 0; base < dim; base += 64) {
        const uint32_t p = base + lane;
        float delta;
        const bool keep = p < dim && delta_kept(x[p], a[p], threshold, &delta);
        count += (uint32_t)__popcll(__ballot(keep));
    }
    if (lane == 0) counts[row] = count;
}

// exclusive scan of the counts into u64 offsets, off[n] = the total: one workgroup walks the rows kScanBlock at a time and carries
// the running total across the blocks
__global__ void __launch_bounds__(kScanBlock) delta_scan_kernel(const uint32_t* __restrict__ counts, uint64_t n, uint64_t* __restrict__ off) {
    __shared__ uint64_t buf[kScanBlock];
    const uint32_t t = threadIdx.x;
    uint64_t carry = 0;
    for (uint64_t base = 0; base < n; base += kScanBlock) {
        const uint64_t i = base + t;
        const uint64_t v = i < n ? counts[i] : 0;
        buf[t] = v;
        __syncthreads();
        for (uint32_t s = 1; s < kScanBlock; s <<= 1) {
            const uint64_t add = t >= s ? buf[t - s] : 0;
            __syncthreads();
            buf[t] += add;
            __syncthreads();
        }
        if (i < n) off[i] = carry + buf[t] - v;
        carry += buf[kScanBlock - 1];
        __syncthreads();
    }
    if (t == 0) off[n] = carry;
}

// pass 2: the same walk; a lane's slot is the row's offset + the entries of earlier steps + the kept lanes below it, so the entries
// land in position order.  Ordinary vector stores.
__global__ void __launch_bounds__(256) delta_write_kernel(const float* __restrict__ rows, uint64_t n, uint32_t dim,
                                                          const float* __restrict__ arch, const int64_t* __restrict__ ids, float threshold,
                                                          const uint64_t* __restrict__ off, uint64_t cap, uint16_t* __restrict__ pos,
                                                          float* __restrict__ del) {
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t row = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= n) return;
    const float* x = rows + row * dim;
    const float* a = arch + (uint64_t)ids[row] * dim;
    uint64_t at = off[row];
    for (uint32_t base = 0; base < dim; base += 64) {
        const uint32_t p = base + lane;
        float delta = 0.0f;
        const bool keep = p < dim && delta_kept(x[p], a[p], threshold, &delta);
        const uint64_t mask = __ballot(keep);
        if (keep) {
            const uint64_t slot = at + (uint64_t)__popcll(mask & ((1ull << lane) - 1ull));
            if (slot < cap) {  // (always: cap is off[n] of the same counts)
                pos[slot] = (uint16_t)p;
                del[slot] = delta;
            }
        }
        at += (uint64_t)__popcll(mask);
    }
}

// scratch[q][a] = dot(archetype a, query q) for a < K, scratch[q][K] = sqrt(sum q * q): nq x (K + 1) chains, a thread each
__global__ void __launch_bounds__(256) delta_arch_dot_kernel(const float* __restrict__ arch, uint32_t K, uint32_t dim,
                                                             const float* __restrict__ queries, uint32_t nq, float* __restrict__ scratch) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (uint64_t)nq * (K + 1)) return;
    const uint32_t q = (uint32_t)(i / (K + 1)), a = (uint32_t)(i % (K + 1));
    const float* qv = queries + (uint64_t)q * dim;
    scratch[i] = a < K ? chain_dot(arch + (uint64_t)a * dim, qv, dim) : sqrtf(chain_sq(qv, dim));
}

// dot_dense / cosine_similarity_dense of a 64-row slice with one query: a lane per row walks its own entries in stored order in the
// slice's entry-major copy (entry e of lane l at slice_off + e * 64 + l) and stops at its own length: padding is never touched.
__global__ void __launch_bounds__(64) delta_score_kernel(const uint32_t* __restrict__ aid, const uint64_t* __restrict__ indptr,
                                                         const uint64_t* __restrict__ slice_off, const uint16_t* __restrict__ spos,
                                                         const float* __restrict__ sdel, const float* __restrict__ mags, uint64_t n,
                                                         uint32_t dim, uint32_t K, const float* __restrict__ queries,
                                                         const float* __restrict__ scratch, int cosine, int query_in_lds,
                                                         float* __restrict__ out) {
    extern __shared__ float qs[];
    const uint32_t lane = threadIdx.x, q = blockIdx.y;
    const uint64_t slice = blockIdx.x, row = slice * 64 + lane;
    const float* qv = queries + (uint64_t)q * dim;
    if (query_in_lds) {
        for (uint32_t d = lane; d < dim; d += 64) qs[d] = qv[d];
        __syncthreads();
    }
    if (row >= n) return;
    const uint64_t len = indptr[row + 1] - indptr[row];
    const uint64_t base = slice_off[slice] + lane;
    const float delta_dot = query_in_lds ? gather_dot(spos + base, sdel + base, len, 64, qs) : gather_dot(spos + base, sdel + base, len, 64, qv);
    const float* sc = scratch + (uint64_t)q * (K + 1);
    const float dot = sc[aid[row]] + delta_dot;
    out[(uint64_t)q * n + row] = cosine ? cosine_of(dot, mags[row], sc[K]) : dot;
}

// to_dense of rows [row0, row0 + gridDim.x): a wave per row copies the archetype; a row whose positions strictly ascend scatters its
// entries in parallel (no two meet), any other row keeps its order on lane 0.
__global__ void __launch_bounds__(64) delta_decode_kernel(const uint32_t* __restrict__ aid, const uint64_t* __restrict__ indptr,
                                                          const uint16_t* __restrict__ pos, const float* __restrict__ del,
                                                          const uint8_t* __restrict__ sorted, const float* __restrict__ arch, uint32_t dim,
                                                          uint64_t row0, float* __restrict__ out) {
    const uint32_t lane = threadIdx.x;
    const uint64_t row = row0 + blockIdx.x;
    const float* a = arch + (uint64_t)aid[row] * dim;
    float* o = out + (uint64_t)blockIdx.x * dim;
    const uint64_t b = indptr[row], e = indptr[row + 1];
    for (uint32_t d = lane; d < dim; d += 64) o[d] = a[d];
    __syncthreads();
    if (sorted[row]) {
        for (uint64_t i = b + lane; i < e; i += 64) o[pos[i]] = a[pos[i]] + del[i];
    } else if (lane == 0) {
        apply_deltas(pos + b, del + b, e - b, o);
    }
}

// magnitude of the rows without a cached value: a thread per decoded row of the tile runs sqrt(sum x * x)
__global__ void __launch_bounds__(256) delta_magnitude_kernel(const float* __restrict__ dense, uint64_t rows, uint32_t dim, uint64_t row0,
                                                              const uint8_t* __restrict__ has_cached, float* __restrict__ mags) {
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= rows || has_cached[row0 + r]) return;
    mags[row0 + r] = sqrtf(chain_sq(dense + r * dim, dim));
}

// dot_deltas_same_archetype: a thread per pair
__global__ void __launch_bounds__(256) delta_pair_kernel(const uint32_t* __restrict__ aid_a, const uint64_t* __restrict__ ptr_a,
                                                         const uint16_t* __restrict__ pos_a, const float* __restrict__ del_a,
                                                         const uint32_t* __restrict__ aid_b, const uint64_t* __restrict__ ptr_b,
                                                         const uint16_t* __restrict__ pos_b, const float* __restrict__ del_b,
                                                         const float* __restrict__ arch, const float* __restrict__ msq, uint32_t dim,
                                                         const uint64_t* __restrict__ pairs, uint64_t n_pairs, float* __restrict__ out,
                                                         uint8_t* __restrict__ ok) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_pairs) return;
    const uint64_t ra = pairs[2 * i], rb = pairs[2 * i + 1];
    const uint32_t id = aid_a[ra];
    if (id != aid_b[rb]) {
        ok[i] = 0;
        return;
    }
    ok[i] = 1;
    out[i] = pair_dot(pos_a + ptr_a[ra], del_a + ptr_a[ra], ptr_a[ra + 1] - ptr_a[ra], pos_b + ptr_b[rb], del_b + ptr_b[rb],
                      ptr_b[rb + 1] - ptr_b[rb], arch + (uint64_t)id * dim, msq[id]);
}

// ---- top-k over a set's scores (docs/delta.md §8) -----------------------------------------------------------------------------

// four score words of one query from the 16-byte aligned word v0 of `al`: the words [a0, vend) are the query's, a word outside
// them is never read and gives kKeyMasked (score_to_key itself never returns it); one 16-byte load where all four are the query's
__device__ __forceinline__ void load_keys4(const uint32_t* __restrict__ al, uint64_t v0, uint32_t a0, uint64_t vend, uint32_t key[4]) {
    if (v0 >= a0 && v0 + 4 <= vend) {
        const uint4 w = *reinterpret_cast<const uint4*>(al + v0);
        key[0] = score_to_key(u2f(w.x));
        key[1] = score_to_key(u2f(w.y));
        key[2] = score_to_key(u2f(w.z));
        key[3] = score_to_key(u2f(w.w));
    } else {
#pragma unroll
        for (uint32_t u = 0; u < 4; u++) {
            const uint64_t v = v0 + u;
            key[u] = v >= a0 && v < vend ? score_to_key(u2f(al[v])) : kKeyMasked;
        }
    }
}

// The first min(k, n) rows of one query's n scores under (key descending, row ascending), k <= kSelectMaxK: a workgroup per query
// (the grid's x).  Three histogram passes over the key bits 31-21, 20-10 and 9-0, each within the bin found before, give the exact
// k-th key T, the keys above it and the keys equal to it; a fourth pass collects every row above T in any order and the first
// (k - above) rows AT T in row order (the chunks ascend, a thread's four rows ascend, and a block-wide prefix of the tie counts
// ranks them; where every tie is wanted no rank is needed); then a bitonic sort of the composites key << 32 | ~row in LDS.  The
// score written is the row's own word, not key_to_score of its key: a -0.0 stays -0.0 and a NaN keeps its payload.
__global__ void __launch_bounds__(kSelThreads) deltaset_select_kernel(const uint32_t* __restrict__ scores, uint64_t n, uint32_t k,
                                                                      uint64_t* __restrict__ out_rows, uint32_t* __restrict__ out_scores,
                                                                      uint32_t* __restrict__ out_counts) {
    __shared__ uint32_t hist[kBins];
    __shared__ unsigned long long list[kSelectMaxK];
    __shared__ PickResult pick;
    __shared__ uint32_t n_list;
    __shared__ uint32_t wsum[kSelThreads / 64];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint64_t q = blockIdx.x;
    const uint32_t* sc = scores + q * n;
    const uint32_t a0 = (uint32_t)((reinterpret_cast<uintptr_t>(sc) >> 2) & 3u);  // words between the 16-byte border below and sc
    const uint32_t* al = sc - a0;
    const uint64_t vend = (uint64_t)a0 + n;
    const uint32_t kk = (uint32_t)(n < (uint64_t)k ? n : (uint64_t)k);  // the rows that answer
    uint32_t prefix = 0, need = kk, above = 0, eq_total = 0;
    uint32_t key[4];
    if (kk) {
        for (int pass = 0; pass < 3; pass++) {
            for (uint32_t i = tid; i < (uint32_t)kBins; i += kSelThreads) hist[i] = 0;
            __syncthreads();
            for (uint64_t c0 = 0; c0 < vend; c0 += kSelectChunk) {
                load_keys4(al, c0 + tid * 4, a0, vend, key);
#pragma unroll
                for (uint32_t u = 0; u < 4; u++) {
                    bool in = key[u] != kKeyMasked;
                    uint32_t bin = key[u] >> 21;
                    if (pass == 1) in = in && (key[u] >> 21) == prefix, bin = (key[u] >> 10) & 2047u;
                    if (pass == 2) in = in && (key[u] >> 10) == prefix, bin = key[u] & 1023u;
                    hist_add_wave(hist, in, bin);
                }
            }
            __syncthreads();
            pick_bin(hist, pass == 2 ? 1024 : kBins, need, &pick);
            const uint32_t bin = pick.bin;
            if (pass == 2) eq_total = hist[bin];  // the bin of the last pass is one key: the rows that hold T
            prefix = pass == 0 ? bin : (prefix << (pass == 1 ? 11 : 10)) | bin;
            above += pick.above;
            need -= pick.above;
            __syncthreads();
        }
    }
    const uint32_t T = prefix;
    if (tid == 0) n_list = 0;
    __syncthreads();
    if (kk) {
        const bool ranked = eq_total > need;  // more rows at T than are wanted: the lowest rows win
        uint32_t running = 0;                 // rows at T in the chunks before this one
        for (uint64_t c0 = 0; c0 < vend; c0 += kSelectChunk) {
            const uint64_t v0 = c0 + tid * 4;
            load_keys4(al, v0, a0, vend, key);
            uint32_t ties = 0;
#pragma unroll
            for (uint32_t u = 0; u < 4; u++) {
                const bool tie = key[u] == T;
                ties += tie ? 1u : 0u;
                const uint32_t slot = wave_append(key[u] > T || (tie && !ranked), &n_list);
                if (slot < kSelectMaxK)
                    list[slot] = ((unsigned long long)key[u] << 32) | (uint32_t)~(uint32_t)(v0 + u - a0);
            }
            if (ranked && running < need) {  // (uniform: `running` is the same in every thread)
                uint32_t incl = ties;
                for (int off = 1; off < 64; off <<= 1) {
                    const uint32_t t = __shfl_up(incl, off);
                    if (lane >= (uint32_t)off) incl += t;
                }
                if (lane == 63) wsum[wave] = incl;
                __syncthreads();
                uint32_t before = 0, total = 0;
                for (uint32_t w = 0; w < kSelThreads / 64; w++) {
                    before += w < wave ? wsum[w] : 0u;
                    total += wsum[w];
                }
                uint32_t rank = running + before + incl - ties;
#pragma unroll
                for (uint32_t u = 0; u < 4; u++) {
                    if (key[u] == T) {
                        if (rank < need) list[above + rank] = ((unsigned long long)T << 32) | (uint32_t)~(uint32_t)(v0 + u - a0);
                        rank++;
                    }
                }
                running += total;
                __syncthreads();
            }
        }
    }
    uint32_t P = 2;
    while (P < kk) P <<= 1;
    __syncthreads();
    for (uint32_t i = kk + tid; i < P; i += kSelThreads) list[i] = 0ull;  // padding sorts last
    __syncthreads();
    for (uint32_t stage = 2; stage <= P; stage <<= 1) {
        for (uint32_t j = stage >> 1; j > 0; j >>= 1) {
            for (uint32_t p = tid; p < P / 2; p += kSelThreads) {
                const uint32_t i = ((p & ~(j - 1)) << 1) | (p & (j - 1));
                const unsigned long long x = list[i], y = list[i + j];
                if ((i & stage) == 0 ? x < y : x > y) {
                    list[i] = y;
                    list[i + j] = x;
                }
            }
            __syncthreads();
        }
    }
    for (uint32_t i = tid; i < k; i += kSelThreads) {
        uint64_t row = UINT64_MAX;
        uint32_t word = 0xFF800000u;  // -inf
        if (i < kk) {
            const uint32_t r = ~(uint32_t)list[i];
            row = r;
            word = sc[r];
        }
        out_rows[q * k + i] = row;
        out_scores[q * k + i] = word;
    }
    if (tid == 0) out_counts[q] = kk;
}

// the large-k path reads a word of all ones as "this row does not take part"; as a score it is one more NaN.  Any other NaN takes
// its place in the copy that is ranked (every NaN ranks alike); the scores that are returned are gathered from the original.
__global__ void __launch_bounds__(256) deltaset_rank_words_kernel(const uint32_t* __restrict__ in, uint64_t n, uint32_t* __restrict__ out) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x)
        out[i] = in[i] == kScoreSentinelBits ? 0x7FC00000u : in[i];
}

__global__ void __launch_bounds__(256) deltaset_gather_kernel(const uint32_t* __restrict__ scores, const uint64_t* __restrict__ rows, uint32_t k,
                                                              uint32_t* __restrict__ out_scores) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < k; i += (uint64_t)gridDim.x * blockDim.x)
        if (rows[i] != UINT64_MAX) out_scores[i] = scores[rows[i]];
}

// ---- sets made on the device (docs/delta.md §9) -------------------------------------------------------------------------------

// exclusive scan of u32 counts into u64 offsets, off[n] = the total, for the whole of a set at once: one 1024-thread workgroup,
// the scan inside a wave by shuffles, one LDS hop across the 16 waves, the running total carried across the blocks of 1024
__global__ void __launch_bounds__(kSelThreads) deltaset_scan_kernel(const uint32_t* __restrict__ counts, uint64_t n, uint64_t* __restrict__ off) {
    __shared__ unsigned long long wtot[kSelThreads / 64];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    unsigned long long carry = 0;
    for (uint64_t base = 0; base < n; base += kSelThreads) {
        const uint64_t i = base + tid;
        const unsigned long long v = i < n ? counts[i] : 0;
        unsigned long long incl = v;
        for (int d = 1; d < 64; d <<= 1) {
            const unsigned long long t = __shfl_up(incl, d);
            if (lane >= (uint32_t)d) incl += t;
        }
        if (lane == 63) wtot[wave] = incl;
        __syncthreads();
        unsigned long long before = 0, total = 0;
        for (uint32_t w = 0; w < kSelThreads / 64; w++) {
            before += w < wave ? wtot[w] : 0ull;
            total += wtot[w];
        }
        if (i < n) off[i] = carry + before + incl - v;
        carry += total;
        __syncthreads();
    }
    if (tid == 0) off[n] = carry;
}

// a wave per 64-row slice: 64 x the longest of its rows, the entries the slice takes in the entry-major copy (<= 64 x 65535)
__global__ void __launch_bounds__(256) deltaset_slice_len_kernel(const uint64_t* __restrict__ indptr, uint64_t n, uint64_t nslices,
                                                                 uint32_t* __restrict__ out) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t slice = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (slice >= nslices) return;  // a whole wave leaves together
    const uint64_t row = slice * 64 + lane;
    uint32_t len = row < n ? (uint32_t)(indptr[row + 1] - indptr[row]) : 0u;
    for (int d = 32; d > 0; d >>= 1) len = max(len, (uint32_t)__shfl_xor((int)len, d));
    if (lane == 0) out[slice] = len * 64u;
}

// a wave per row: entry e of row r goes to slice_off[r / 64] + e * 64 + r % 64; the padding was zeroed before
__global__ void __launch_bounds__(256) deltaset_slice_write_kernel(const uint64_t* __restrict__ indptr, const uint16_t* __restrict__ pos,
                                                                   const float* __restrict__ del, const uint64_t* __restrict__ slice_off,
                                                                   uint64_t n, uint16_t* __restrict__ spos, float* __restrict__ sdel) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t row = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= n) return;
    const uint64_t p0 = indptr[row], len = indptr[row + 1] - p0, base = slice_off[row >> 6] + (row & 63u);
    for (uint64_t e = lane; e < len; e += 64) {  // (base + e * 64 < slice_off[r / 64 + 1]: the slice is as long as its longest row)
        spos[base + e * 64] = pos[p0 + e];
        sdel[base + e * 64] = del[p0 + e];
    }
}

__global__ void __launch_bounds__(256) deltaset_aid_kernel(const int64_t* __restrict__ ids, uint64_t n, uint32_t* __restrict__ aid) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) aid[i] = (uint32_t)ids[i];
}

// a chunk's offsets into the set's: indptr[i] = base + off[i] for i <= m
__global__ void __launch_bounds__(256) deltaset_rebase_kernel(const uint64_t* __restrict__ off, uint64_t m, uint64_t base, uint64_t* __restrict__ indptr) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i <= m; i += (uint64_t)gridDim.x * blockDim.x) indptr[i] = base + off[i];
}

// ---- host helpers -----------------------------------------------------------------------------------------------------------

template <class F>
void parallel_rows(uint64_t n, uint64_t work_per_row, F&& fn) {
    unsigned threads = std::thread::hardware_concurrency();
    threads = threads ? std::min(threads, 16u) : 1u;
    if (n * std::max<uint64_t>(work_per_row, 1) < (1u << 16)) threads = 1;
    threads = (unsigned)std::min<uint64_t>(threads, std::max<uint64_t>(n, 1));
    if (threads <= 1) {
        fn((uint64_t)0, n);
        return;
    }
    std::vector<std::thread> pool;
    const uint64_t per = (n + threads - 1) / threads;
    for (unsigned t = 0; t < threads; t++) {
        const uint64_t b = std::min<uint64_t>(n, t * per), e = std::min<uint64_t>(n, b + per);
        if (b < e) pool.emplace_back([&fn, b, e] { fn(b, e); });
    }
    for (auto& th : pool) th.join();
}

struct DevBuf {  // a device allocation that frees itself
    void* p = nullptr;
    ~DevBuf() {
        if (p) (void)hipFree(p);
    }
    hipError_t alloc(size_t bytes) { return hipMalloc(&p, bytes ? bytes : 4); }
    template <class T>
    T* as() const {
        return static_cast<T*>(p);
    }
};

#define D_TRY(expr)                                          \
    do {                                                     \
        hipError_t _e = (expr);                              \
        if (_e != hipSuccess) return set_error_hip(_e, #expr); \
    } while (0)

std::string dimension_exceeded(uint64_t dim) {  // DeltaVectorError::DimensionExceeded, Display (53-61)
    return "dimension " + std::to_string(dim) + " exceeds maximum " + std::to_string(NMN_DELTA_MAX_DIMENSION) + " (u16::MAX)";
}

}  // namespace

// ---- handles ----------------------------------------------------------------------------------------------------------------

struct nmn_archetypes {
    uint32_t dim = 0;
    uint64_t max = 0;
    int device = -1;
    std::atomic<uint64_t> min_device_rows{UINT64_MAX};
    std::shared_mutex rw;      // the registry's contents
    std::vector<float> rows;   // [len][dim]
    std::vector<float> msq;    // magnitude_sq
    std::mutex gpu;            // the device mirror and the handle's stream: one host-buffer call at a time uses the device
    hipStream_t stream = nullptr;
    float* d_rows = nullptr;   // [d_count][dim]
    float* d_msq = nullptr;
    // archetypes in the mirror; the registry only appends, so count == len means current.  Written under `gpu`, read by the
    // stream-ordered forms without it: atomic, released after the arrays they describe are in place
    std::atomic<uint64_t> d_count{0};
    std::atomic<bool> d_valid{false};
    uint64_t len() const { return msq.size(); }
};

struct nmn_delta_set {
    nmn_archetypes* reg = nullptr;
    uint64_t n = 0;
    std::vector<uint32_t> aid;
    std::vector<uint64_t> indptr;  // [n + 1]
    std::vector<uint16_t> pos;
    std::vector<float> del;
    std::vector<float> cached;
    std::vector<uint8_t> has, sorted;
    // device mirror (under reg->gpu): the CSR arrays, the 64-row entry-major slices, and every row's magnitude
    std::atomic<bool> resident{false};  // written under reg->gpu, read by the stream-ordered forms without it
    uint32_t* d_aid = nullptr;
    uint64_t* d_indptr = nullptr;
    uint16_t* d_pos = nullptr;
    float* d_del = nullptr;
    uint8_t* d_has = nullptr;
    uint8_t* d_sorted = nullptr;
    uint64_t* d_slice_off = nullptr;
    uint16_t* d_spos = nullptr;
    float* d_sdel = nullptr;
    float* d_mag = nullptr;
    // a set made on the device (docs/delta.md §9) holds no host copy of the seven arrays above until something asks for one:
    // ensure_host downloads each once, at its final size, under host_mx.  nnz is stored; `ready` is recorded on the stream that
    // built the mirror, and the library's own calls wait for it; temps are the builder's device temporaries, freed once it is done
    uint64_t nnz = 0;
    bool with_magnitude = false;
    std::atomic<bool> host_present{true};
    std::mutex host_mx;
    hipEvent_t ready = nullptr;
    std::vector<void*> temps;
    void free_temps() {
        for (void* p : temps) (void)hipFree(p);
        temps.clear();
    }
    void free_device() {
        free_temps();
        for (void* p : {(void*)d_aid, (void*)d_indptr, (void*)d_pos, (void*)d_del, (void*)d_has, (void*)d_sorted, (void*)d_slice_off,
                        (void*)d_spos, (void*)d_sdel, (void*)d_mag})
            if (p) (void)hipFree(p);
        d_aid = nullptr, d_indptr = nullptr, d_pos = nullptr, d_del = nullptr, d_has = nullptr, d_sorted = nullptr;
        d_slice_off = nullptr, d_spos = nullptr, d_sdel = nullptr, d_mag = nullptr;
        resident = false;
    }
};

namespace {

bool on_device(const nmn_archetypes* a, uint64_t rows) { return rows >= a->min_device_rows.load(std::memory_order_relaxed); }

nmn_status use_device(nmn_archetypes* a) {
    if (a->device >= 0) D_TRY(hipSetDevice(a->device));
    if (!a->stream) D_TRY(hipStreamCreateWithFlags(&a->stream, hipStreamNonBlocking));
    return NMN_OK;
}

// the registry's mirror; caller holds a->rw (shared or unique) and a->gpu
nmn_status registry_to_device(nmn_archetypes* a) {
    nmn_status st = use_device(a);
    if (st != NMN_OK) return st;
    if (a->d_valid && a->d_count == a->len()) return NMN_OK;
    D_TRY(hipStreamSynchronize(a->stream));
    if (a->d_rows) (void)hipFree(a->d_rows);
    if (a->d_msq) (void)hipFree(a->d_msq);
    a->d_rows = nullptr, a->d_msq = nullptr, a->d_valid = false;
    const size_t K = a->len();
    D_TRY(hipMalloc(reinterpret_cast<void**>(&a->d_rows), std::max<size_t>(K * a->dim, 1) * 4));
    D_TRY(hipMalloc(reinterpret_cast<void**>(&a->d_msq), std::max<size_t>(K, 1) * 4));
    if (K) {
        D_TRY(hipMemcpy(a->d_rows, a->rows.data(), K * a->dim * 4, hipMemcpyHostToDevice));
        D_TRY(hipMemcpy(a->d_msq, a->msq.data(), K * 4, hipMemcpyHostToDevice));
    }
    a->d_count = K;
    a->d_valid = true;
    return NMN_OK;
}

uint64_t chunk_rows(uint32_t dim) { return std::max<uint64_t>(64, (kChunkBytes / 4 / dim) & ~63ull); }

void launch_find_best(nmn_archetypes* a, const float* rows_dev, uint64_t n, int64_t* ids, float* sims, float* mags, hipStream_t s) {
    hipLaunchKernelGGL(delta_find_best_kernel, dim3((uint32_t)((n + 63) / 64)), dim3(64), 0, s, rows_dev, n, a->dim, a->d_rows, a->d_msq,
                       (uint32_t)a->d_count, ids, sims, mags);
}

// find_best_archetype of host rows; mags (nullable) = sqrt(sum x * x).  Caller holds a->rw; the registry is not empty.
nmn_status find_best_rows(nmn_archetypes* a, const float* rows, uint64_t n, int64_t* ids, float* sims, float* mags) {
    const uint32_t dim = a->dim;
    const uint64_t K = a->len();
    if (!on_device(a, n)) {
        parallel_rows(n, (uint64_t)dim * K, [&](uint64_t b, uint64_t e) {
            for (uint64_t i = b; i < e; i++) {
                const float* x = rows + i * dim;
                const float query_mag = sqrtf(chain_sq(x, dim));
                if (mags) mags[i] = query_mag;
                int64_t best_id = 0;
                float best_sim = -INFINITY;
                if (query_mag == 0.0f) {
                    best_sim = 0.0f;
                } else {
                    for (uint64_t id = 0; id < K; id++) {
                        const float sim = arch_sim(chain_dot(a->rows.data() + id * dim, x, dim), a->msq[id], query_mag);
                        if (sim > best_sim) {
                            best_sim = sim;
                            best_id = (int64_t)id;
                        }
                    }
                }
                if (ids) ids[i] = best_id;
                if (sims) sims[i] = best_sim;
            }
        });
        return NMN_OK;
    }
    std::lock_guard<std::mutex> g(a->gpu);
    nmn_status st = registry_to_device(a);
    if (st != NMN_OK) return st;
    const uint64_t ch = std::min(chunk_rows(dim), std::max<uint64_t>(n, 1));
    DevBuf d_x, d_ids, d_sims, d_mags;
    D_TRY(d_x.alloc(ch * dim * 4));
    D_TRY(d_ids.alloc(ch * 8));
    D_TRY(d_sims.alloc(ch * 4));
    D_TRY(d_mags.alloc(ch * 4));
    for (uint64_t r0 = 0; r0 < n; r0 += ch) {
        const uint64_t m = std::min(ch, n - r0);
        D_TRY(hipMemcpyAsync(d_x.p, rows + r0 * dim, m * dim * 4, hipMemcpyHostToDevice, a->stream));
        launch_find_best(a, d_x.as<float>(), m, d_ids.as<int64_t>(), d_sims.as<float>(), d_mags.as<float>(), a->stream);
        D_TRY(hipGetLastError());
        if (ids) D_TRY(hipMemcpyAsync(ids + r0, d_ids.p, m * 8, hipMemcpyDeviceToHost, a->stream));
        if (sims) D_TRY(hipMemcpyAsync(sims + r0, d_sims.p, m * 4, hipMemcpyDeviceToHost, a->stream));
        if (mags) D_TRY(hipMemcpyAsync(mags + r0, d_mags.p, m * 4, hipMemcpyDeviceToHost, a->stream));
        D_TRY(hipStreamSynchronize(a->stream));
    }
    return NMN_OK;
}

// encode of host rows: ids, nnz per row and (want_entries) the entries appended to pos / del in row order.  Caller holds a->rw.
nmn_status encode_rows(nmn_archetypes* a, const float* rows, uint64_t n, float threshold, std::vector<int64_t>& ids, std::vector<float>& sims,
                       std::vector<float>& mags, std::vector<uint64_t>& indptr, bool want_entries, std::vector<uint16_t>& pos,
                       std::vector<float>& del) {
    const uint32_t dim = a->dim;
    ids.assign(n, 0);
    sims.assign(n, 0.0f);
    mags.assign(n, 0.0f);
    indptr.assign(n + 1, 0);
    pos.clear();
    del.clear();
    if (!on_device(a, n)) {
        nmn_status st = find_best_rows(a, rows, n, ids.data(), sims.data(), mags.data());
        if (st != NMN_OK) return st;
        std::vector<uint32_t> counts(n);
        parallel_rows(n, dim, [&](uint64_t b, uint64_t e) {
            for (uint64_t i = b; i < e; i++) {
                const float* x = rows + i * dim;
                const float* r = a->rows.data() + (uint64_t)ids[i] * dim;
                uint32_t c = 0;
                float d;
                for (uint32_t p = 0; p < dim; p++) c += delta_kept(x[p], r[p], threshold, &d) ? 1u : 0u;
                counts[i] = c;
            }
        });
        for (uint64_t i = 0; i < n; i++) indptr[i + 1] = indptr[i] + counts[i];
        if (!want_entries) return NMN_OK;
        pos.resize(indptr[n]);
        del.resize(indptr[n]);
        parallel_rows(n, dim, [&](uint64_t b, uint64_t e) {
            for (uint64_t i = b; i < e; i++) {
                const float* x = rows + i * dim;
                const float* r = a->rows.data() + (uint64_t)ids[i] * dim;
                uint64_t at = indptr[i];
                float d;
                for (uint32_t p = 0; p < dim; p++)
                    if (delta_kept(x[p], r[p], threshold, &d)) {
                        pos[at] = (uint16_t)p;
                        del[at++] = d;
                    }
            }
        });
        return NMN_OK;
    }
    std::lock_guard<std::mutex> g(a->gpu);
    nmn_status st = registry_to_device(a);
    if (st != NMN_OK) return st;
    hipStream_t s = a->stream;
    const uint64_t ch = std::min(chunk_rows(dim), std::max<uint64_t>(n, 1));
    DevBuf d_x, d_ids, d_sims, d_mags, d_counts, d_off;
    D_TRY(d_x.alloc(ch * dim * 4));
    D_TRY(d_ids.alloc(ch * 8));
    D_TRY(d_sims.alloc(ch * 4));
    D_TRY(d_mags.alloc(ch * 4));
    D_TRY(d_counts.alloc(ch * 4));
    D_TRY(d_off.alloc((ch + 1) * 8));
    std::vector<uint64_t> off(ch + 1);
    for (uint64_t r0 = 0; r0 < n; r0 += ch) {
        const uint64_t m = std::min(ch, n - r0);
        const uint32_t wave_blocks = (uint32_t)((m + 3) / 4);
        D_TRY(hipMemcpyAsync(d_x.p, rows + r0 * dim, m * dim * 4, hipMemcpyHostToDevice, s));
        launch_find_best(a, d_x.as<float>(), m, d_ids.as<int64_t>(), d_sims.as<float>(), d_mags.as<float>(), s);
        hipLaunchKernelGGL(delta_count_kernel, dim3(wave_blocks), dim3(256), 0, s, d_x.as<float>(), m, dim, a->d_rows, d_ids.as<int64_t>(),
                           threshold, d_counts.as<uint32_t>());
        hipLaunchKernelGGL(delta_scan_kernel, dim3(1), dim3(kScanBlock), 0, s, d_counts.as<uint32_t>(), m, d_off.as<uint64_t>());
        D_TRY(hipGetLastError());
        D_TRY(hipMemcpyAsync(off.data(), d_off.p, (m + 1) * 8, hipMemcpyDeviceToHost, s));
        D_TRY(hipMemcpyAsync(ids.data() + r0, d_ids.p, m * 8, hipMemcpyDeviceToHost, s));
        D_TRY(hipMemcpyAsync(sims.data() + r0, d_sims.p, m * 4, hipMemcpyDeviceToHost, s));
        D_TRY(hipMemcpyAsync(mags.data() + r0, d_mags.p, m * 4, hipMemcpyDeviceToHost, s));
        D_TRY(hipStreamSynchronize(s));
        const uint64_t base = indptr[r0], total = off[m];
        for (uint64_t i = 0; i < m; i++) indptr[r0 + i + 1] = base + off[i + 1];
        if (!want_entries || total == 0) continue;
        DevBuf d_pos, d_del;
        D_TRY(d_pos.alloc(total * 2));
        D_TRY(d_del.alloc(total * 4));
        hipLaunchKernelGGL(delta_write_kernel, dim3(wave_blocks), dim3(256), 0, s, d_x.as<float>(), m, dim, a->d_rows, d_ids.as<int64_t>(),
                           threshold, d_off.as<uint64_t>(), total, d_pos.as<uint16_t>(), d_del.as<float>());
        D_TRY(hipGetLastError());
        pos.resize(base + total);
        del.resize(base + total);
        D_TRY(hipMemcpyAsync(pos.data() + base, d_pos.p, total * 2, hipMemcpyDeviceToHost, s));
        D_TRY(hipMemcpyAsync(del.data() + base, d_del.p, total * 4, hipMemcpyDeviceToHost, s));
        D_TRY(hipStreamSynchronize(s));
    }
    return NMN_OK;
}

float ratio_of(uint32_t dim, uint64_t nnz) {  // compression_ratio (410-416)
    const uint64_t dense_bytes = (uint64_t)dim * 4;
    if (dense_bytes == 0) return 1.0f;
    const uint64_t memory_bytes = NMN_DELTA_VECTOR_BYTES + nnz * 2 + nnz * 4;
    return (float)dense_bytes / (float)memory_bytes;
}

template <class T>
hipError_t upload(T** dst, const std::vector<T>& v) {
    hipError_t e = hipMalloc(reinterpret_cast<void**>(dst), std::max<size_t>(v.size(), 1) * sizeof(T));
    if (e == hipSuccess && !v.empty()) e = hipMemcpy(*dst, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice);
    return e;
}

// the set's mirror; caller holds reg->rw (shared) and reg->gpu, and the registry's mirror is current
nmn_status set_to_device(nmn_delta_set* s) {
    if (s->resident) {  // a set made on the device, perhaps on a stream of the caller's: a host-buffer call waits for its end
        if (s->ready) D_TRY(hipEventSynchronize(s->ready));
        return NMN_OK;
    }
    nmn_archetypes* a = s->reg;
    const uint64_t n = s->n;
    const uint32_t dim = a->dim;
    const uint64_t nslices = (n + 63) / 64;
    std::vector<uint64_t> slice_off(nslices + 1, 0);
    for (uint64_t sl = 0; sl < nslices; sl++) {
        uint64_t longest = 0;
        for (uint64_t r = sl * 64; r < std::min(n, sl * 64 + 64); r++) longest = std::max(longest, s->indptr[r + 1] - s->indptr[r]);
        slice_off[sl + 1] = slice_off[sl] + longest * 64;
    }
    std::vector<uint16_t> spos(slice_off[nslices], 0);
    std::vector<float> sdel(slice_off[nslices], 0.0f);
    parallel_rows(n, 64, [&](uint64_t b, uint64_t e) {
        for (uint64_t r = b; r < e; r++) {
            const uint64_t base = slice_off[r / 64] + r % 64, p0 = s->indptr[r], len = s->indptr[r + 1] - p0;
            for (uint64_t k = 0; k < len; k++) {
                spos[base + k * 64] = s->pos[p0 + k];
                sdel[base + k * 64] = s->del[p0 + k];
            }
        }
    });
    auto fail = [&](hipError_t e) {
        s->free_device();
        return set_error_hip(e, "nmn_delta_set: device mirror");
    };
    hipError_t e = upload(&s->d_aid, s->aid);
    if (e == hipSuccess) e = upload(&s->d_indptr, s->indptr);
    if (e == hipSuccess) e = upload(&s->d_pos, s->pos);
    if (e == hipSuccess) e = upload(&s->d_del, s->del);
    if (e == hipSuccess) e = upload(&s->d_has, s->has);
    if (e == hipSuccess) e = upload(&s->d_sorted, s->sorted);
    if (e == hipSuccess) e = upload(&s->d_slice_off, slice_off);
    if (e == hipSuccess) e = upload(&s->d_spos, spos);
    if (e == hipSuccess) e = upload(&s->d_sdel, sdel);
    if (e == hipSuccess) e = upload(&s->d_mag, s->cached);
    if (e != hipSuccess) return fail(e);
    // the rows without a cached magnitude: decode a tile of rows, then one chain per row
    uint64_t first = n;
    for (uint64_t r = 0; r < n; r++)
        if (!s->has[r]) {
            first = r;
            break;
        }
    if (first < n) {
        const uint64_t tile = std::min<uint64_t>(n - first, std::max<uint64_t>(64, (64ull << 20) / 4 / dim));
        DevBuf dense;
        e = dense.alloc(tile * dim * 4);
        for (uint64_t r0 = first; r0 < n && e == hipSuccess; r0 += tile) {
            const uint64_t m = std::min(tile, n - r0);
            hipLaunchKernelGGL(delta_decode_kernel, dim3((uint32_t)m), dim3(64), 0, a->stream, s->d_aid, s->d_indptr, s->d_pos, s->d_del,
                               s->d_sorted, a->d_rows, dim, r0, dense.as<float>());
            hipLaunchKernelGGL(delta_magnitude_kernel, dim3((uint32_t)((m + 255) / 256)), dim3(256), 0, a->stream, dense.as<float>(), m, dim, r0,
                               s->d_has, s->d_mag);
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = hipStreamSynchronize(a->stream);
        if (e != hipSuccess) return fail(e);
    }
    s->resident = true;
    return NMN_OK;
}

// both mirrors for a host-buffer call; caller holds reg->rw (shared) and reg->gpu
nmn_status mirrors(nmn_delta_set* s) {
    nmn_status st = registry_to_device(s->reg);
    return st == NMN_OK ? set_to_device(s) : st;
}

// the host arrays of a set made on the device, on first need: each array once, at its final size, under the set's lock (two
// threads asking together get one download).  The values are those encode_batch has always returned: cached = 0.0 and has = 0
// without with_magnitude, sorted = 1 throughout.
nmn_status ensure_host(nmn_delta_set* s) {
    if (s->host_present.load(std::memory_order_acquire)) return NMN_OK;
    std::lock_guard<std::mutex> g(s->host_mx);
    if (s->host_present.load(std::memory_order_acquire)) return NMN_OK;
    nmn_archetypes* a = s->reg;
    if (a->device >= 0) D_TRY(hipSetDevice(a->device));
    if (s->ready) D_TRY(hipEventSynchronize(s->ready));
    s->free_temps();
    const uint64_t n = s->n;
    s->aid.resize(n);
    s->indptr.resize(n + 1);
    s->pos.resize(s->nnz);
    s->del.resize(s->nnz);
    s->cached.assign(n, 0.0f);
    s->has.assign(n, s->with_magnitude ? 1 : 0);
    s->sorted.assign(n, 1);
    D_TRY(hipMemcpy(s->aid.data(), s->d_aid, n * 4, hipMemcpyDeviceToHost));
    D_TRY(hipMemcpy(s->indptr.data(), s->d_indptr, (n + 1) * 8, hipMemcpyDeviceToHost));
    if (s->nnz) {
        D_TRY(hipMemcpy(s->pos.data(), s->d_pos, s->nnz * 2, hipMemcpyDeviceToHost));
        D_TRY(hipMemcpy(s->del.data(), s->d_del, s->nnz * 4, hipMemcpyDeviceToHost));
    }
    if (s->with_magnitude) D_TRY(hipMemcpy(s->cached.data(), s->d_mag, n * 4, hipMemcpyDeviceToHost));  // every row's magnitude is its cached one
    s->host_present.store(true, std::memory_order_release);
    return NMN_OK;
}

uint32_t stream_grid(uint64_t n) { return (uint32_t)std::min<uint64_t>(std::max<uint64_t>((n + 255) / 256, 1), 8192); }

template <class T>
hipError_t dev_alloc(T** p, uint64_t count) {
    return hipMalloc(reinterpret_cast<void**>(p), std::max<uint64_t>(count, 1) * sizeof(T));
}

// encode n rows into a resident set without a host copy (docs/delta.md §9).  rows_host: the rows go up in chunks on `st`;
// rows_dev: they are where they are.  Enqueues find_best, count and scan per chunk, the slice lengths and their scan, then WAITS once
// for two u64 — the entry total and the slice total — (with more than one chunk: once per chunk for its entry total, then once
// for the slice total), allocates, and enqueues the entry write, the slice write and the magnitudes; the set's event ends it.
// Caller holds a->rw; the registry's mirror is current and not empty; n >= 1, dim <= 65535.
nmn_status encode_resident(nmn_archetypes* a, const float* rows_host, const float* rows_dev, uint64_t n, float threshold, bool with_magnitude,
                           int64_t* ids_out_dev, float* sims_out_dev, hipStream_t st, nmn_delta_set* s) {
    const uint32_t dim = a->dim;
    const uint64_t ch = rows_dev ? n : std::min(chunk_rows(dim), n);
    const uint64_t nslices = (n + 63) / 64;
    auto fail = [&](hipError_t e, const char* what) {
        (void)hipStreamSynchronize(st);
        s->free_device();
        return set_error_hip(e, what);
    };
#define E_TRY(expr)                                   \
    do {                                              \
        hipError_t _e = (expr);                       \
        if (_e != hipSuccess) return fail(_e, #expr); \
    } while (0)
    float* d_x = nullptr;
    int64_t* d_ids = ids_out_dev;
    uint32_t *d_counts = nullptr, *d_slen = nullptr;
    uint64_t* d_off = nullptr;
    auto temp = [&](auto** p, uint64_t count) {
        hipError_t e = dev_alloc(p, count);
        if (e == hipSuccess) s->temps.push_back(*p);
        return e;
    };
    if (rows_host) E_TRY(temp(&d_x, ch * dim));
    if (!d_ids) E_TRY(temp(&d_ids, n));
    E_TRY(temp(&d_counts, ch));
    E_TRY(temp(&d_slen, nslices));
    E_TRY(dev_alloc(&s->d_mag, n));
    E_TRY(dev_alloc(&s->d_indptr, n + 1));
    E_TRY(dev_alloc(&s->d_slice_off, nslices + 1));
    E_TRY(dev_alloc(&s->d_aid, n));
    E_TRY(dev_alloc(&s->d_has, n));
    E_TRY(dev_alloc(&s->d_sorted, n));
    const bool one = ch >= n;  // one chunk: its offsets are the set's, and the one wait brings both totals
    if (!one) E_TRY(temp(&d_off, ch + 1));
    struct Piece {
        uint16_t* pos;
        float* del;
        uint64_t total;
    };
    std::vector<Piece> pieces;
    uint64_t totals[2] = {0, 0}, base = 0;
    auto slices = [&]() {
        hipLaunchKernelGGL(deltaset_slice_len_kernel, dim3((uint32_t)((nslices + 3) / 4)), dim3(256), 0, st, s->d_indptr, n, nslices, d_slen);
        hipLaunchKernelGGL(deltaset_scan_kernel, dim3(1), dim3(kSelThreads), 0, st, d_slen, nslices, s->d_slice_off);
    };
    for (uint64_t r0 = 0; r0 < n; r0 += ch) {
        const uint64_t m = std::min(ch, n - r0);
        const uint32_t wave_blocks = (uint32_t)((m + 3) / 4);
        const float* x = rows_dev ? rows_dev : d_x;
        if (rows_host) E_TRY(hipMemcpyAsync(d_x, rows_host + r0 * dim, m * dim * 4, hipMemcpyHostToDevice, st));
        launch_find_best(a, x, m, d_ids + r0, sims_out_dev ? sims_out_dev + r0 : nullptr, s->d_mag + r0, st);
        hipLaunchKernelGGL(delta_count_kernel, dim3(wave_blocks), dim3(256), 0, st, x, m, dim, a->d_rows, d_ids + r0, threshold, d_counts);
        uint64_t* off = one ? s->d_indptr : d_off;
        hipLaunchKernelGGL(deltaset_scan_kernel, dim3(1), dim3(kSelThreads), 0, st, d_counts, m, off);
        if (one) slices();
        E_TRY(hipGetLastError());
        E_TRY(hipMemcpyAsync(&totals[0], off + m, 8, hipMemcpyDeviceToHost, st));
        if (one) E_TRY(hipMemcpyAsync(&totals[1], s->d_slice_off + nslices, 8, hipMemcpyDeviceToHost, st));
        E_TRY(hipStreamSynchronize(st));  // the one wait (per chunk)
        Piece p{nullptr, nullptr, totals[0]};
        E_TRY(dev_alloc(&p.pos, p.total));
        pieces.push_back(p);
        E_TRY(dev_alloc(&pieces.back().del, p.total));
        p = pieces.back();
        hipLaunchKernelGGL(delta_write_kernel, dim3(wave_blocks), dim3(256), 0, st, x, m, dim, a->d_rows, d_ids + r0, threshold, off, p.total, p.pos,
                           p.del);
        if (!one) hipLaunchKernelGGL(deltaset_rebase_kernel, dim3(stream_grid(m + 1)), dim3(256), 0, st, off, m, base, s->d_indptr + r0);
        E_TRY(hipGetLastError());
        base += p.total;
    }
    s->nnz = base;
    if (one) {
        s->d_pos = pieces[0].pos, s->d_del = pieces[0].del;
        pieces.clear();
    } else {  // join the pieces device to device
        hipError_t e = dev_alloc(&s->d_pos, base);
        if (e == hipSuccess) e = dev_alloc(&s->d_del, base);
        uint64_t at = 0;
        for (const Piece& p : pieces) {
            if (e == hipSuccess && p.total) e = hipMemcpyAsync(s->d_pos + at, p.pos, p.total * 2, hipMemcpyDeviceToDevice, st);
            if (e == hipSuccess && p.total) e = hipMemcpyAsync(s->d_del + at, p.del, p.total * 4, hipMemcpyDeviceToDevice, st);
            at += p.total;
            s->temps.push_back(p.pos);
            s->temps.push_back(p.del);
        }
        pieces.clear();
        if (e != hipSuccess) return fail(e, "nmn_delta_set: joining the chunks");
        slices();
        E_TRY(hipGetLastError());
        E_TRY(hipMemcpyAsync(&totals[1], s->d_slice_off + nslices, 8, hipMemcpyDeviceToHost, st));
        E_TRY(hipStreamSynchronize(st));
    }
    const uint64_t slice_total = totals[1];
    E_TRY(dev_alloc(&s->d_spos, slice_total));
    E_TRY(dev_alloc(&s->d_sdel, slice_total));
    if (slice_total) {  // padding is zero, as the host builder leaves it
        E_TRY(hipMemsetAsync(s->d_spos, 0, slice_total * 2, st));
        E_TRY(hipMemsetAsync(s->d_sdel, 0, slice_total * 4, st));
    }
    E_TRY(hipMemsetAsync(s->d_has, with_magnitude ? 1 : 0, n, st));
    E_TRY(hipMemsetAsync(s->d_sorted, 1, n, st));
    hipLaunchKernelGGL(deltaset_aid_kernel, dim3(stream_grid(n)), dim3(256), 0, st, d_ids, n, s->d_aid);
    hipLaunchKernelGGL(deltaset_slice_write_kernel, dim3((uint32_t)((n + 3) / 4)), dim3(256), 0, st, s->d_indptr, s->d_pos, s->d_del, s->d_slice_off, n,
                       s->d_spos, s->d_sdel);
    E_TRY(hipGetLastError());
    if (!with_magnitude) {  // sqrt(sum) over the reconstruction, not over the input: decode a tile of rows, then one chain per row
        const uint64_t tile = std::min<uint64_t>(n, std::max<uint64_t>(64, (64ull << 20) / 4 / dim));
        float* dense = nullptr;
        E_TRY(temp(&dense, tile * dim));
        for (uint64_t r0 = 0; r0 < n; r0 += tile) {
            const uint64_t m = std::min(tile, n - r0);
            hipLaunchKernelGGL(delta_decode_kernel, dim3((uint32_t)m), dim3(64), 0, st, s->d_aid, s->d_indptr, s->d_pos, s->d_del, s->d_sorted, a->d_rows,
                               dim, r0, dense);
            hipLaunchKernelGGL(delta_magnitude_kernel, dim3((uint32_t)((m + 255) / 256)), dim3(256), 0, st, dense, m, dim, r0, s->d_has, s->d_mag);
        }
        E_TRY(hipGetLastError());
    }
    E_TRY(hipEventCreateWithFlags(&s->ready, hipEventDisableTiming));
    E_TRY(hipEventRecord(s->ready, st));
#undef E_TRY
    s->n = n;
    s->with_magnitude = with_magnitude;
    s->host_present.store(false, std::memory_order_release);
    s->resident = true;
    return NMN_OK;
}

void host_decode_row(const nmn_delta_set* s, uint64_t r, float* out) {
    const uint32_t dim = s->reg->dim;
    memcpy(out, s->reg->rows.data() + (uint64_t)s->aid[r] * dim, (size_t)dim * 4);
    apply_deltas(s->pos.data() + s->indptr[r], s->del.data() + s->indptr[r], s->indptr[r + 1] - s->indptr[r], out);
}

void host_magnitudes(const nmn_delta_set* s, float* out) {
    const uint32_t dim = s->reg->dim;
    parallel_rows(s->n, dim, [&](uint64_t b, uint64_t e) {
        std::vector<float> dense(dim);
        for (uint64_t r = b; r < e; r++) {
            if (s->has[r]) {
                out[r] = s->cached[r];
                continue;
            }
            host_decode_row(s, r, dense.data());
            out[r] = sqrtf(chain_sq(dense.data(), dim));
        }
    });
}

void launch_score(nmn_delta_set* s, const float* q_dev, uint32_t nq, float* scratch, int cosine, float* out, hipStream_t st) {
    nmn_archetypes* a = s->reg;
    const uint32_t K = (uint32_t)a->d_count, dim = a->dim;
    const int in_lds = dim <= kLdsQueryDim;
    for (uint32_t q0 = 0; q0 < nq; q0 += kQueryBlock) {  // a block of queries per launch: the grid's y is 16 bits wide
        const uint32_t m = nq - q0 < kQueryBlock ? nq - q0 : kQueryBlock;
        const float* qb = q_dev + (uint64_t)q0 * dim;
        float* sb = scratch + (uint64_t)q0 * (K + 1);
        const uint64_t chains = (uint64_t)m * (K + 1);
        hipLaunchKernelGGL(delta_arch_dot_kernel, dim3((uint32_t)((chains + 255) / 256)), dim3(256), 0, st, a->d_rows, K, dim, qb, m, sb);
        hipLaunchKernelGGL(delta_score_kernel, dim3((uint32_t)((s->n + 63) / 64), m), dim3(64), in_lds ? (size_t)dim * 4 : 0, st, s->d_aid,
                           s->d_indptr, s->d_slice_off, s->d_spos, s->d_sdel, s->d_mag, s->n, dim, K, qb, sb, cosine, in_lds,
                           out + (uint64_t)q0 * s->n);
    }
}

nmn_status score(nmn_delta_set* s, const float* queries, uint32_t nq, int cosine, float* out) {
    if (!s || (!queries && nq) || (!out && nq)) return set_error(NMN_ERR_INVALID_ARGUMENT, "null argument");
    nmn_archetypes* a = s->reg;
    const uint64_t n = s->n;
    const uint32_t dim = a->dim;
    if (n == 0 || nq == 0) return NMN_OK;
    std::shared_lock<std::shared_mutex> lk(a->rw);
    if (!on_device(a, n)) {
        { nmn_status hs = ensure_host(s); if (hs != NMN_OK) return hs; }
        const uint64_t K = a->len();
        std::vector<float> arch_dot((size_t)nq * (K + 1));
        parallel_rows((uint64_t)nq * (K + 1), dim, [&](uint64_t b, uint64_t e) {
            for (uint64_t i = b; i < e; i++) {
                const float* qv = queries + (i / (K + 1)) * dim;
                const uint64_t id = i % (K + 1);
                arch_dot[i] = id < K ? chain_dot(a->rows.data() + id * dim, qv, dim) : sqrtf(chain_sq(qv, dim));
            }
        });
        std::vector<float> mags;
        if (cosine) {
            mags.resize(n);
            host_magnitudes(s, mags.data());
        }
        parallel_rows(n, (uint64_t)nq * 16, [&](uint64_t b, uint64_t e) {
            for (uint32_t q = 0; q < nq; q++) {
                const float* qv = queries + (uint64_t)q * dim;
                const float* sc = arch_dot.data() + (uint64_t)q * (K + 1);
                for (uint64_t r = b; r < e; r++) {
                    const uint64_t p0 = s->indptr[r];
                    const float dot = sc[s->aid[r]] + gather_dot(s->pos.data() + p0, s->del.data() + p0, s->indptr[r + 1] - p0, 1, qv);
                    out[(uint64_t)q * n + r] = cosine ? cosine_of(dot, mags[r], sc[K]) : dot;
                }
            }
        });
        return NMN_OK;
    }
    std::lock_guard<std::mutex> g(a->gpu);
    nmn_status st = mirrors(s);
    if (st != NMN_OK) return st;
    DevBuf d_q, d_scratch, d_out;
    D_TRY(d_q.alloc((size_t)nq * dim * 4));
    D_TRY(d_scratch.alloc((size_t)nq * (a->d_count + 1) * 4));
    D_TRY(d_out.alloc((size_t)nq * n * 4));
    D_TRY(hipMemcpyAsync(d_q.p, queries, (size_t)nq * dim * 4, hipMemcpyHostToDevice, a->stream));
    launch_score(s, d_q.as<float>(), nq, d_scratch.as<float>(), cosine, d_out.as<float>(), a->stream);
    D_TRY(hipGetLastError());
    D_TRY(hipMemcpyAsync(out, d_out.p, (size_t)nq * n * 4, hipMemcpyDeviceToHost, a->stream));
    D_TRY(hipStreamSynchronize(a->stream));
    return NMN_OK;
}

nmn_status score_device(nmn_delta_set* s, const float* q_dev, uint32_t nq, float* scratch, float* out, int cosine, void* stream) {
    if (!s || !q_dev || !scratch || !out) return set_error(NMN_ERR_INVALID_ARGUMENT, "null argument");
    nmn_archetypes* a = s->reg;
    std::shared_lock<std::shared_mutex> lk(a->rw);
    if (!a->d_valid || a->d_count != a->len())
        return set_error(NMN_ERR_INVALID_ARGUMENT, "the registry is not resident on the device: call nmn_archetypes_to_device after the last register");
    if (!s->resident) return set_error(NMN_ERR_INVALID_ARGUMENT, "the delta set is not resident on the device: call nmn_delta_set_to_device first");
    if (s->n == 0 || nq == 0) return NMN_OK;
    if (a->device >= 0) D_TRY(hipSetDevice(a->device));
    launch_score(s, q_dev, nq, scratch, cosine, out, static_cast<hipStream_t>(stream));
    D_TRY(hipGetLastError());
    return NMN_OK;
}

// ---- top-k search -----------------------------------------------------------------------------------------------------------

uint64_t align256(uint64_t bytes) { return (bytes + 255) & ~255ull; }

// Which of the two selections answers.  The select kernel is one workgroup per query, so a single query over a large set keeps
// one CU busy while the sort of the large-k path uses the whole device: measured (docs/delta.md §7), one query over 200 000 rows
// costs the same either way and over 1M rows the sort is 2.3 times faster.  Two queries over 1M rows are still 27 % faster
// through two sorts and are NOT routed: the rule is one query, as measured, not a model of queries x sort time.
bool search_sorts(uint64_t n, uint32_t nq, uint32_t k) { return k > kSelectMaxK || (nq == 1 && n >= kSortSingleRows); }

// the device scratch of a search of nq queries at once over n rows against K archetypes: the archetype dots, the score words, and
// where the sort answers the ranked copy of one query's words and the sort keys of the large-k path
struct SearchScratch {
    uint64_t arch_dot = 0, scores = 0, words = 0, keys = 0, bytes = 0;
    SearchScratch(uint64_t n, uint64_t K, uint32_t nq, uint32_t k) {
        const bool sorts = search_sorts(n, nq, k);
        scores = arch_dot + align256((uint64_t)nq * (K + 1) * 4);
        words = scores + align256((uint64_t)nq * n * 4);
        keys = words + (sorts ? align256(n * 4) : 0);
        bytes = keys + (sorts ? largek_sort_len(n) * 8 : 0);
    }
};

nmn_status search_refusals(const nmn_delta_set* s, uint32_t k) {
    if (k == 0) return set_error(NMN_ERR_INVALID_ARGUMENT, "a top-k search needs k of at least 1");
    if (s->n >= 0xFFFFFFFFull)
        return set_error(NMN_ERR_INVALID_ARGUMENT, "a top-k search serves a delta set of at most 4294967294 rows: the row is the low half of a sort key");
    return NMN_OK;
}

// score and select nq <= nq_laid queries (DEVICE) on `st`; the set and its registry are resident.  base: scratch of
// SearchScratch(n, K, nq_laid, k), and nq_laid chooses the selection with it: the scratch of the sort is there or it is not
hipError_t launch_search(nmn_delta_set* s, const float* q_dev, uint32_t nq, uint32_t nq_laid, uint32_t k, int cosine, char* base,
                         uint64_t* rows_dev, float* scores_dev, uint32_t* counts_dev, hipStream_t st) {
    const uint64_t n = s->n;
    const SearchScratch sc(n, s->reg->d_count, nq_laid, k);
    uint32_t* words = reinterpret_cast<uint32_t*>(base + sc.scores);
    if (n) launch_score(s, q_dev, nq, reinterpret_cast<float*>(base + sc.arch_dot), cosine, reinterpret_cast<float*>(words), st);
    if (!search_sorts(n, nq_laid, k) || n == 0) {  // (no rows: the kernel reads none and writes the unused slots)
        hipLaunchKernelGGL(deltaset_select_kernel, dim3(nq), dim3(kSelThreads), 0, st, words, n, k, rows_dev, reinterpret_cast<uint32_t*>(scores_dev),
                           counts_dev);
        return hipGetLastError();
    }
    uint32_t* ranked = reinterpret_cast<uint32_t*>(base + sc.words);
    const uint32_t grid_n = (uint32_t)std::min<uint64_t>((n + 255) / 256, 8192), grid_k = (uint32_t)std::min<uint64_t>(((uint64_t)k + 255) / 256, 8192);
    for (uint32_t q = 0; q < nq; q++) {  // the sort of the large-k path, one query at a time: the same order by construction
        const uint32_t* w = words + (uint64_t)q * n;
        hipLaunchKernelGGL(deltaset_rank_words_kernel, dim3(grid_n), dim3(256), 0, st, w, n, ranked);
        hipError_t e = launch_largek(ranked, n, reinterpret_cast<uint64_t*>(base + sc.keys), k, 0, rows_dev + (uint64_t)q * k,
                                     scores_dev + (uint64_t)q * k, counts_dev + q, st);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(deltaset_gather_kernel, dim3(grid_k), dim3(256), 0, st, w, rows_dev + (uint64_t)q * k, k,
                           reinterpret_cast<uint32_t*>(scores_dev + (uint64_t)q * k));
    }
    return hipGetLastError();
}

// the queries one step of a host-buffer search takes: their score words and their answers each stay within kSearchBudget
uint32_t search_block(uint64_t n, uint32_t nq, uint32_t k) {
    const uint64_t by_scores = kSearchBudget / std::max<uint64_t>(n * 4, 1), by_answers = kSearchBudget / ((uint64_t)k * 12);
    return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(nq, std::min(by_scores, by_answers)));
}

nmn_status search(nmn_delta_set* s, const float* queries, uint32_t nq, uint32_t k, int cosine, uint64_t* rows_out, float* scores_out,
                  uint32_t* counts_out) {
    if (!s) return set_error(NMN_ERR_INVALID_ARGUMENT, "null argument");
    nmn_status st = search_refusals(s, k);
    if (st != NMN_OK) return st;
    if (nq && (!queries || !rows_out || !scores_out || !counts_out)) return set_error(NMN_ERR_INVALID_ARGUMENT, "null argument");
    if (nq == 0) return NMN_OK;
    nmn_archetypes* a = s->reg;
    const uint64_t n = s->n;
    const uint32_t dim = a->dim;
    const uint32_t kk = (uint32_t)std::min<uint64_t>(k, n);
    const uint32_t qb = search_block(n, nq, k);
    if (n == 0 || !on_device(a, n)) {
        // the host scores, then a partial sort of the composites key << 32 | ~row: the same key and the same tie rule
        std::vector<float> sc((size_t)qb * n);
        for (uint32_t q0 = 0; q0 < nq; q0 += qb) {
            const uint32_t m = std::min(qb, nq - q0);
            if (n) {
                st = score(s, queries + (uint64_t)q0 * dim, m, cosine, sc.data());
                if (st != NMN_OK) return st;
            }
            parallel_rows(m, n * 8, [&](uint64_t b, uint64_t e) {
                std::vector<uint64_t> comp(n);
                for (uint64_t q = b; q < e; q++) {
                    const float* row_scores = sc.data() + q * n;
                    for (uint64_t r = 0; r < n; r++) comp[r] = ((uint64_t)score_to_key(row_scores[r]) << 32) | (uint32_t)~(uint32_t)r;
                    std::partial_sort(comp.begin(), comp.begin() + kk, comp.end(), std::greater<uint64_t>());
                    uint64_t* ro = rows_out + (q0 + q) * k;
                    float* so = scores_out + (q0 + q) * k;
                    for (uint32_t i = 0; i < k; i++) {
                        const uint32_t unused = 0xFF800000u;  // -inf
                        if (i < kk) {
                            const uint32_t r = ~(uint32_t)comp[i];
                            ro[i] = r;
                            memcpy(so + i, row_scores + r, 4);  // the row's own bits
                        } else {
                            ro[i] = UINT64_MAX;
                            memcpy(so + i, &unused, 4);
                        }
                    }
                    counts_out[q0 + q] = kk;
                }
            });
        }
        return NMN_OK;
    }
    std::shared_lock<std::shared_mutex> lk(a->rw);
    std::lock_guard<std::mutex> g(a->gpu);
    st = mirrors(s);
    if (st != NMN_OK) return st;
    const SearchScratch lay(n, a->d_count, qb, k);
    DevBuf d_q, d_scratch, d_rows, d_sc, d_counts;
    D_TRY(d_q.alloc((size_t)qb * dim * 4));
    D_TRY(d_scratch.alloc(lay.bytes));
    D_TRY(d_rows.alloc((size_t)qb * k * 8));
    D_TRY(d_sc.alloc((size_t)qb * k * 4));
    D_TRY(d_counts.alloc((size_t)qb * 4));
    for (uint32_t q0 = 0; q0 < nq; q0 += qb) {
        const uint32_t m = std::min(qb, nq - q0);
        D_TRY(hipMemcpyAsync(d_q.p, queries + (uint64_t)q0 * dim, (size_t)m * dim * 4, hipMemcpyHostToDevice, a->stream));
        // (the layout of qb queries serves a last, shorter block too: launch_search lays out m queries within it)
        D_TRY(launch_search(s, d_q.as<float>(), m, qb, k, cosine, d_scratch.as<char>(), d_rows.as<uint64_t>(), d_sc.as<float>(), d_counts.as<uint32_t>(),
                            a->stream));
        D_TRY(hipMemcpyAsync(rows_out + (uint64_t)q0 * k, d_rows.p, (size_t)m * k * 8, hipMemcpyDeviceToHost, a->stream));
        D_TRY(hipMemcpyAsync(scores_out + (uint64_t)q0 * k, d_sc.p, (size_t)m * k * 4, hipMemcpyDeviceToHost, a->stream));
        D_TRY(hipMemcpyAsync(counts_out + q0, d_counts.p, (size_t)m * 4, hipMemcpyDeviceToHost, a->stream));
        D_TRY(hipStreamSynchronize(a->stream));
    }
    return NMN_OK;
}

nmn_status search_device(nmn_delta_set* s, const float* q_dev, uint32_t nq, uint32_t k, int cosine, void* scratch, uint64_t scratch_bytes,
                         uint64_t* rows_dev, float* scores_dev, uint32_t* counts_dev, void* stream) {
    if (!s) return set_error(NMN_ERR_INVALID_ARGUMENT, "null argument");
    nmn_status st = search_refusals(s, k);
    if (st != NMN_OK) return st;
    if (!q_dev || !scratch || !rows_dev || !scores_dev || !counts_dev) return set_error(NMN_ERR_INVALID_ARGUMENT, "null argument");
    nmn_archetypes* a = s->reg;
    std::shared_lock<std::shared_mutex> lk(a->rw);
    if (!a->d_valid || a->d_count != a->len())
        return set_error(NMN_ERR_INVALID_ARGUMENT, "the registry is not resident on the device: call nmn_archetypes_to_device after the last register");
    if (!s->resident) return set_error(NMN_ERR_INVALID_ARGUMENT, "the delta set is not resident on the device: call nmn_delta_set_to_device first");
    if (reinterpret_cast<uintptr_t>(scratch) & 15u) return set_error(NMN_ERR_INVALID_ARGUMENT, "the search scratch must be aligned to 16 bytes");
    const uint64_t want = SearchScratch(s->n, a->d_count, nq, k).bytes;
    if (scratch_bytes < want)
        return set_error(NMN_ERR_INVALID_ARGUMENT, ("the search scratch holds " + std::to_string(scratch_bytes) + " bytes, the search needs " +
                                                    std::to_string(want) + " (nmn_deltaset_search_scratch_bytes)")
                                                       .c_str());
    if (nq == 0) return NMN_OK;
    if (a->device >= 0) D_TRY(hipSetDevice(a->device));
    D_TRY(launch_search(s, q_dev, nq, nq, k, cosine, static_cast<char*>(scratch), rows_dev, scores_dev, counts_dev, static_cast<hipStream_t>(stream)));
    return NMN_OK;
}

}  // namespace

// ---- C ABI ------------------------------------------------------------------------------------------------------------------

extern "C" void nmn_delta_options_default(nmn_delta_options* opt) {
    if (opt) opt->min_device_rows = NMN_DELTA_DEFAULT_MIN_DEVICE_ROWS;
}

extern "C" nmn_status nmn_delta_limits(uint32_t* max_dimension, uint32_t* lds_query_dim, uint32_t* archetype_tile, uint32_t* scan_block) {
    if (max_dimension) *max_dimension = NMN_DELTA_MAX_DIMENSION;
    if (lds_query_dim) *lds_query_dim = kLdsQueryDim;
    if (archetype_tile) *archetype_tile = kArchTile;
    if (scan_block) *scan_block = kScanBlock;
    return NMN_OK;
}

extern "C" nmn_status nmn_archetypes_create(uint32_t dim, uint64_t max_archetypes, int32_t device, nmn_archetypes** out) {
    if (!out) return set_error(NMN_ERR_INVALID_ARGUMENT, "null argument");
    *out = nullptr;
    if (dim == 0) return set_error(NMN_ERR_INVALID_ARGUMENT, "an archetype registry needs a dimension of at least 1");
    if (max_archetypes > 0xFFFFFFFFull) return set_error(NMN_ERR_INVALID_ARGUMENT, "max_archetypes is above the limit of 4294967295");
    nmn_archetypes* a = new nmn_archetypes();
    a->dim = dim;
    a->max = max_archetypes;
    a->device = device;
    nmn_delta_options opt;
    nmn_delta_options_default(&opt);
    a->min_device_rows = opt.min_device_rows;
    *out = a;
    return NMN_OK;
}

extern "C" nmn_status nmn_archetypes_destroy(nmn_archetypes* a) {
    if (!a) return NMN_OK;
    if (a->stream || a->d_rows) {
        if (a->device >= 0) (void)hipSetDevice(a->device);
        if (a->stream) {
            (void)hipStreamSynchronize(a->stream);
            (void)hipStreamDestroy(a->stream);
        }
        if (a->d_rows) (void)hipFree(a->d_rows);
        if (a->d_msq) (void)hipFree(a->d_msq);
    }
    delete a;
    return NMN_OK;
}

extern "C" nmn_status nmn_archetypes_set_options(nmn_archetypes* a, const nmn_delta_options* opt) {
    if (!a || !opt) return set_error(NMN_ERR_INVALID_ARGUMENT, "null argument");
    a->min_device_rows = opt->min_device_rows;
    return NMN_OK;
}

extern "C" nmn_status nmn_archetypes_register(nmn_archetypes* a, const float* rows, uint64_t n, int64_t* ids_out) {
    if (!a || (!rows && n)) return set_error(NMN_ERR_INVALID_ARGUMENT, "null argument");
    std::unique_lock<std::shared_mutex> lk(a->rw);
    for (uint64_t i = 0; i < n; i++) {
        if (a->len() >= a->max) {  // `return None`
            if (ids_out) ids_out[i] = -1;
            continue;
        }
        const float* x = rows + i * a->dim;
        if (ids_out) ids_out[i] = (int64_t)a->len();
        a->rows.insert(a->rows.end(), x, x + a->dim);
        a->msq.push_back(chain_sq(x, a->dim));
    }
    return NMN_OK;
}

extern "C" nmn_status nmn_archetypes_discover(nmn_archetypes* a, const float* rows, uint64_t n, uint64_t k, const nmn_kmeans_options* opt,
                                              uint64_t* added_out) {
    if (!a || (!rows && n) || !opt) return set_error(NMN_ERR_INVALID_ARGUMENT, "null argument");
    if (added_out) *added_out = 0;
    if (n == 0) return NMN_OK;
    uint64_t room;
    {
        std::shared_lock<std::shared_mutex> lk(a->rw);
        room = a->max - std::min<uint64_t>(a->max, a->len());
    }
    k = std::min(std::min(k, n), room);  // `k.min(vectors.len()).min(self.max_archetypes - self.len())`
    if (k == 0) return NMN_OK;
    // KMeans::fit: the exact GPU k-means behind nmn_ivf_build, over a transient flat index
    nmn_index_desc desc{};
    desc.dim = a->dim;
    desc.capacity_rows = n;
    desc.device = a->device;
    nmn_ivf* ivf = nullptr;
    nmn_status st = nmn_ivf_build(&desc, rows, n, (uint32_t)k, opt, &ivf);
    if (st != NMN_OK) return st;
    const uint32_t got = nmn_ivf_clusters(ivf);
    std::vector<float> cents((size_t)got * a->dim);
    st = nmn_ivf_centroids(ivf, cents.data(), cents.size());
    nmn_ivf_destroy(ivf);
    if (st != NMN_OK) return st;
    std::vector<int64_t> ids(got);
    st = nmn_archetypes_register(a, cents.data(), got, ids.data());
    if (st != NMN_OK) return st;
    uint64_t added = 0;
    for (int64_t id : ids) added += id >= 0;
    if (added_out) *added_out = added;
    return NMN_OK;
}

extern "C" uint64_t nmn_archetypes_len(nmn_archetypes* a) {
    if (!a) return 0;
    std::shared_lock<std::shared_mutex> lk(a->rw);
    return a->len();
}
extern "C" uint32_t nmn_archetypes_dim(nmn_archetypes* a) { return a ? a->dim : 0; }
extern "C" uint64_t nmn_archetypes_max(nmn_archetypes* a) { return a ? a->max : 0; }

extern "C" nmn_status nmn_archetypes_get(nmn_archetypes* a, uint64_t id, float* out) {
    if (!a || !out) return set_error(NMN_ERR_INVALID_ARGUMENT, "null argument");
    std::shared_lock<std::shared_mutex> lk(a->rw);
    if (id >= a->len()) return set_error(NMN_ERR_NOT_FOUND, "no archetype with this id");
    memcpy(out, a->rows.data() + id * a->dim, (size_t)a->dim * 4);
    return NMN_OK;
}

extern "C" nmn_status nmn_archetypes_magnitude_sq(nmn_archetypes* a, uint64_t id, float* out) {
    if (!a || !out) return set_error(NMN_ERR_INVALID_ARGUMENT, "null argument");
    std::shared_lock<std::shared_mutex> lk(a->rw);
    if (id >= a->len()) return set_error(NMN_ERR_NOT_FOUND, "no archetype with this id");
    *out = a->msq[id];
    return NMN_OK;
}

extern "C" nmn_status nmn_archetypes_find_best(nmn_archetypes* a, const float* rows, uint64_t n, int64_t* ids_out, float* sims_out) {
    if (!a || (!rows && n)) return set_error(NMN_ERR_INVALID_ARGUMENT, "null argument");
    std::shared_lock<std::shared_mutex> lk(a->rw);
    if (a->len() == 0) {  // `return None`
        for (uint64_t i = 0; ids_out && i < n; i++) ids_out[i] = -1;
        return NMN_OK;
    }
    if (n == 0) return NMN_OK;
    return find_best_rows(a, rows, n, ids_out, sims_out, nullptr);
}

extern "C" nmn_status nmn_archetypes_analyze_coverage(nmn_archetypes* a, const float* rows, uint64_t n, float threshold,
                                                      nmn_coverage_stats* stats_out, uint64_t* usage_out) {
    if (!a || (!rows && n) || !stats_out) return set_error(NMN_ERR_INVALID_ARGUMENT, "null argument");
    std::shared_lock<std::shared_mutex> lk(a->rw);
    memset(stats_out, 0, sizeof *stats_out);
    for (uint64_t i = 0; usage_out && i < a->len(); i++) usage_out[i] = 0;
    if (n == 0 || a->len() == 0) return NMN_OK;  // CoverageStats::default()
    if (a->dim > NMN_DELTA_MAX_DIMENSION) return set_error(NMN_ERR_INVALID_ARGUMENT, dimension_exceeded(a->dim).c_str());
    std::vector<int64_t> ids;
    std::vector<float> sims, mags, del;
    std::vector<uint64_t> indptr;
    std::vector<uint16_t> pos;
    nmn_status st = encode_rows(a, rows, n, threshold, ids, sims, mags, indptr, false, pos, del);
    if (st != NMN_OK) return st;
    float total_similarity = 0.0f, total_compression = 0.0f;  // `let mut total_similarity = 0.0`
    uint64_t total_delta_nnz = 0;
    for (uint64_t i = 0; i < n; i++) {
        const uint64_t nnz = indptr[i + 1] - indptr[i];
        total_similarity = total_similarity + sims[i];
        if (usage_out) usage_out[ids[i]]++;
        total_compression = total_compression + ratio_of(a->dim, nnz);
        total_delta_nnz += nnz;
    }
    const float nf = (float)n;
    stats_out->avg_similarity = total_similarity / nf;
    stats_out->avg_compression_ratio = total_compression / nf;
    stats_out->avg_delta_nnz = (float)total_delta_nnz / nf;
    return NMN_OK;
}

extern "C" nmn_status nmn_archetypes_encode_batch(nmn_archetypes* a, const float* rows, uint64_t n, float threshold, int32_t with_magnitude,
                                                  nmn_delta_set** out) {
    if (!a || (!rows && n) || !out) return set_error(NMN_ERR_INVALID_ARGUMENT, "null argument");
    *out = nullptr;
    std::shared_lock<std::shared_mutex> lk(a->rw);
    // on an empty registry `encode` is None before any DeltaVector is built: an empty set at any dimension, as for no vectors
    if (a->len() != 0 && n != 0 && a->dim > NMN_DELTA_MAX_DIMENSION)
        return set_error(NMN_ERR_INVALID_ARGUMENT, dimension_exceeded(a->dim).c_str());
    nmn_delta_set* s = new nmn_delta_set();
    s->reg = a;
    s->indptr.assign(1, 0);
    if (a->len() != 0 && n != 0 && on_device(a, n)) {
        // the device path: the chunks go up as before, every piece of the CSR stays in HBM and the set is finished there
        std::lock_guard<std::mutex> g(a->gpu);
        nmn_status st = registry_to_device(a);
        if (st == NMN_OK) st = encode_resident(a, rows, nullptr, n, threshold, with_magnitude != 0, nullptr, nullptr, a->stream, s);
        if (st != NMN_OK) {
            delete s;
            return st;
        }
    } else if (a->len() != 0 && n != 0) {
        std::vector<int64_t> ids;
        std::vector<float> sims, mags;
        nmn_status st = encode_rows(a, rows, n, threshold, ids, sims, mags, s->indptr, true, s->pos, s->del);
        if (st != NMN_OK) {
            delete s;
            return st;
        }
        s->n = n;
        s->nnz = s->pos.size();
        s->aid.resize(n);
        for (uint64_t i = 0; i < n; i++) s->aid[i] = (uint32_t)ids[i];
        s->has.assign(n, with_magnitude ? 1 : 0);
        s->sorted.assign(n, 1);
        if (with_magnitude)
            s->cached.swap(mags);
        else
            s->cached.assign(n, 0.0f);
    }
    *out = s;
    return NMN_OK;
}

extern "C" nmn_status nmn_delta_set_from_parts(nmn_archetypes* a, uint64_t n, const uint64_t* archetype_ids, const uint64_t* indptr,
                                               const uint16_t* positions, const float* deltas, const float* cached, const uint8_t* has_cached,
                                               nmn_delta_set** out) {
    if (!a || !out || !indptr || (n && !archetype_ids)) return set_error(NMN_ERR_INVALID_ARGUMENT, "null argument");
    *out = nullptr;
    std::shared_lock<std::shared_mutex> lk(a->rw);
    if (a->dim > NMN_DELTA_MAX_DIMENSION) return set_error(NMN_ERR_INVALID_ARGUMENT, dimension_exceeded(a->dim).c_str());
    if (indptr[0] != 0) return set_error(NMN_ERR_INVALID_ARGUMENT, "delta set: indptr[0] must be 0");
    for (uint64_t i = 0; i < n; i++) {
        if (archetype_ids[i] >= a->len())
            return set_error(NMN_ERR_INVALID_ARGUMENT, ("delta set: row " + std::to_string(i) + ": archetype id " + std::to_string(archetype_ids[i]) +
                                                        " is not registered (the registry holds " + std::to_string(a->len()) + ")")
                                                           .c_str());
        if (indptr[i + 1] < indptr[i])
            return set_error(NMN_ERR_INVALID_ARGUMENT, ("delta set: row " + std::to_string(i) + ": indptr does not ascend").c_str());
    }
    const uint64_t nnz = indptr[n];
    if (nnz && (!positions || !deltas)) return set_error(NMN_ERR_INVALID_ARGUMENT, "null argument");
    nmn_delta_set* s = new nmn_delta_set();
    s->sorted.assign(n, 1);
    for (uint64_t i = 0; i < n; i++)
        for (uint64_t e = indptr[i]; e < indptr[i + 1]; e++) {
            if (positions[e] >= a->dim) {
                delete s;
                return set_error(NMN_ERR_INVALID_ARGUMENT, ("delta set: row " + std::to_string(i) + ": position " + std::to_string(positions[e]) +
                                                            " is not below the dimension " + std::to_string(a->dim))
                                                               .c_str());
            }
            if (e > indptr[i] && positions[e] <= positions[e - 1]) s->sorted[i] = 0;
        }
    s->reg = a;
    s->n = n;
    s->aid.resize(n);
    for (uint64_t i = 0; i < n; i++) s->aid[i] = (uint32_t)archetype_ids[i];
    s->indptr.assign(indptr, indptr + n + 1);
    s->nnz = nnz;
    s->pos.assign(positions, positions + nnz);
    s->del.assign(deltas, deltas + nnz);
    s->has.assign(n, 0);
    s->cached.assign(n, 0.0f);
    for (uint64_t i = 0; cached && i < n; i++)
        if (!has_cached || has_cached[i]) {
            s->has[i] = 1;
            s->cached[i] = cached[i];
        }
    *out = s;
    return NMN_OK;
}

extern "C" nmn_status nmn_delta_set_destroy(nmn_delta_set* s) {
    if (!s) return NMN_OK;
    if (s->d_aid) {
        std::lock_guard<std::mutex> g(s->reg->gpu);
        if (s->reg->device >= 0) (void)hipSetDevice(s->reg->device);
        if (s->ready) {  // a set made on a stream of the caller's: its last kernel has run before its arrays go
            (void)hipEventSynchronize(s->ready);
            (void)hipEventDestroy(s->ready);
        }
        if (s->reg->stream) (void)hipStreamSynchronize(s->reg->stream);
        s->free_device();
    }
    delete s;
    return NMN_OK;
}

extern "C" uint64_t nmn_delta_set_len(nmn_delta_set* s) { return s ? s->n : 0; }
extern "C" uint64_t nmn_delta_set_nnz(nmn_delta_set* s) { return s ? s->nnz : 0; }

extern "C" nmn_status nmn_delta_set_arrays(nmn_delta_set* s, uint64_t* archetype_ids, uint64_t* indptr, uint16_t* positions, float* deltas,
                                           float* cached, uint8_t* has_cached, uint8_t* sorted_out) {
    if (!s) return set_error(NMN_ERR_INVALID_ARGUMENT, "null argument");
    { nmn_status hs = ensure_host(s); if (hs != NMN_OK) return hs; }
    for (uint64_t i = 0; archetype_ids && i < s->n; i++) archetype_ids[i] = s->aid[i];
    if (indptr) memcpy(indptr, s->indptr.data(), (s->n + 1) * 8);
    if (positions && !s->pos.empty()) memcpy(positions, s->pos.data(), s->pos.size() * 2);
    if (deltas && !s->del.empty()) memcpy(deltas, s->del.data(), s->del.size() * 4);
    if (cached && s->n) memcpy(cached, s->cached.data(), s->n * 4);
    if (has_cached && s->n) memcpy(has_cached, s->has.data(), s->n);
    if (sorted_out && s->n) memcpy(sorted_out, s->sorted.data(), s->n);
    return NMN_OK;
}

extern "C" nmn_status nmn_delta_set_compression_ratio(nmn_delta_set* s, float* out) {
    if (!s || (!out && s->n)) return set_error(NMN_ERR_INVALID_ARGUMENT, "null argument");
    { nmn_status hs = ensure_host(s); if (hs != NMN_OK) return hs; }
    for (uint64_t i = 0; i < s->n; i++) out[i] = ratio_of(s->reg->dim, s->indptr[i + 1] - s->indptr[i]);
    return NMN_OK;
}

extern "C" nmn_status nmn_delta_set_memory_bytes(nmn_delta_set* s, uint64_t* out) {
    if (!s || (!out && s->n)) return set_error(NMN_ERR_INVALID_ARGUMENT, "null argument");
    { nmn_status hs = ensure_host(s); if (hs != NMN_OK) return hs; }
    for (uint64_t i = 0; i < s->n; i++) out[i] = NMN_DELTA_VECTOR_BYTES + (s->indptr[i + 1] - s->indptr[i]) * 6;
    return NMN_OK;
}

extern "C" nmn_status nmn_delta_set_decode(nmn_delta_set* s, float* out) {
    if (!s || (!out && s->n)) return set_error(NMN_ERR_INVALID_ARGUMENT, "null argument");
    if (s->n == 0) return NMN_OK;
    nmn_archetypes* a = s->reg;
    const uint32_t dim = a->dim;
    std::shared_lock<std::shared_mutex> lk(a->rw);
    if (!on_device(a, s->n)) {
        { nmn_status hs = ensure_host(s); if (hs != NMN_OK) return hs; }
        parallel_rows(s->n, dim, [&](uint64_t b, uint64_t e) {
            for (uint64_t r = b; r < e; r++) host_decode_row(s, r, out + r * dim);
        });
        return NMN_OK;
    }
    std::lock_guard<std::mutex> g(a->gpu);
    nmn_status st = mirrors(s);
    if (st != NMN_OK) return st;
    const uint64_t tile = std::min(s->n, chunk_rows(dim));
    DevBuf dense;
    D_TRY(dense.alloc(tile * dim * 4));
    for (uint64_t r0 = 0; r0 < s->n; r0 += tile) {
        const uint64_t m = std::min(tile, s->n - r0);
        hipLaunchKernelGGL(delta_decode_kernel, dim3((uint32_t)m), dim3(64), 0, a->stream, s->d_aid, s->d_indptr, s->d_pos, s->d_del, s->d_sorted,
                           a->d_rows, dim, r0, dense.as<float>());
        D_TRY(hipGetLastError());
        D_TRY(hipMemcpyAsync(out + r0 * dim, dense.p, m * dim * 4, hipMemcpyDeviceToHost, a->stream));
        D_TRY(hipStreamSynchronize(a->stream));
    }
    return NMN_OK;
}

extern "C" nmn_status nmn_delta_set_magnitudes(nmn_delta_set* s, float* out) {
    if (!s || (!out && s->n)) return set_error(NMN_ERR_INVALID_ARGUMENT, "null argument");
    if (s->n == 0) return NMN_OK;
    nmn_archetypes* a = s->reg;
    std::shared_lock<std::shared_mutex> lk(a->rw);
    if (!on_device(a, s->n)) {
        { nmn_status hs = ensure_host(s); if (hs != NMN_OK) return hs; }
        host_magnitudes(s, out);
        return NMN_OK;
    }
    std::lock_guard<std::mutex> g(a->gpu);
    nmn_status st = mirrors(s);
    if (st != NMN_OK) return st;
    D_TRY(hipMemcpy(out, s->d_mag, s->n * 4, hipMemcpyDeviceToHost));
    return NMN_OK;
}

extern "C" nmn_status nmn_delta_set_dot_dense(nmn_delta_set* s, const float* queries, uint32_t nq, float* out) {
    return score(s, queries, nq, 0, out);
}
extern "C" nmn_status nmn_delta_set_cosine_dense(nmn_delta_set* s, const float* queries, uint32_t nq, float* out) {
    return score(s, queries, nq, 1, out);
}

extern "C" nmn_status nmn_delta_set_dot_same_archetype(nmn_delta_set* sa, nmn_delta_set* sb, const uint64_t* pairs, uint64_t n_pairs, float* out,
                                                       uint8_t* ok_out) {
    if (!sa || !sb || (n_pairs && (!pairs || !out || !ok_out))) return set_error(NMN_ERR_INVALID_ARGUMENT, "null argument");
    if (sa->reg != sb->reg) return set_error(NMN_ERR_INVALID_ARGUMENT, "the two delta sets belong to different registries");
    for (uint64_t i = 0; i < n_pairs; i++)
        if (pairs[2 * i] >= sa->n || pairs[2 * i + 1] >= sb->n)
            return set_error(NMN_ERR_INVALID_ARGUMENT, ("delta pairs: pair " + std::to_string(i) + " names a row its set does not hold").c_str());
    if (n_pairs == 0) return NMN_OK;
    nmn_archetypes* a = sa->reg;
    const uint32_t dim = a->dim;
    std::shared_lock<std::shared_mutex> lk(a->rw);
    if (!on_device(a, n_pairs)) {
        for (nmn_delta_set* s : {sa, sb}) {
            nmn_status hs = ensure_host(s);
            if (hs != NMN_OK) return hs;
        }
        parallel_rows(n_pairs, 64, [&](uint64_t b, uint64_t e) {
            for (uint64_t i = b; i < e; i++) {
                const uint64_t ra = pairs[2 * i], rb = pairs[2 * i + 1];
                const uint32_t id = sa->aid[ra];
                ok_out[i] = id == sb->aid[rb];
                if (!ok_out[i]) continue;
                out[i] = pair_dot(sa->pos.data() + sa->indptr[ra], sa->del.data() + sa->indptr[ra], sa->indptr[ra + 1] - sa->indptr[ra],
                                  sb->pos.data() + sb->indptr[rb], sb->del.data() + sb->indptr[rb], sb->indptr[rb + 1] - sb->indptr[rb],
                                  a->rows.data() + (uint64_t)id * dim, a->msq[id]);
            }
        });
        return NMN_OK;
    }
    std::lock_guard<std::mutex> g(a->gpu);
    nmn_status st = mirrors(sa);
    if (st == NMN_OK) st = set_to_device(sb);
    if (st != NMN_OK) return st;
    DevBuf d_pairs, d_out, d_ok;
    D_TRY(d_pairs.alloc(n_pairs * 16));
    D_TRY(d_out.alloc(n_pairs * 4));
    D_TRY(d_ok.alloc(n_pairs));
    D_TRY(hipMemcpyAsync(d_pairs.p, pairs, n_pairs * 16, hipMemcpyHostToDevice, a->stream));
    D_TRY(hipMemcpyAsync(d_out.p, out, n_pairs * 4, hipMemcpyHostToDevice, a->stream));  // a None leaves out[i] as it was
    hipLaunchKernelGGL(delta_pair_kernel, dim3((uint32_t)((n_pairs + 255) / 256)), dim3(256), 0, a->stream, sa->d_aid, sa->d_indptr, sa->d_pos,
                       sa->d_del, sb->d_aid, sb->d_indptr, sb->d_pos, sb->d_del, a->d_rows, a->d_msq, dim, d_pairs.as<uint64_t>(), n_pairs,
                       d_out.as<float>(), d_ok.as<uint8_t>());
    D_TRY(hipGetLastError());
    D_TRY(hipMemcpyAsync(out, d_out.p, n_pairs * 4, hipMemcpyDeviceToHost, a->stream));
    D_TRY(hipMemcpyAsync(ok_out, d_ok.p, n_pairs, hipMemcpyDeviceToHost, a->stream));
    D_TRY(hipStreamSynchronize(a->stream));
    return NMN_OK;
}

extern "C" nmn_status nmn_archetypes_to_device(nmn_archetypes* a) {
    if (!a) return set_error(NMN_ERR_INVALID_ARGUMENT, "null argument");
    std::shared_lock<std::shared_mutex> lk(a->rw);
    std::lock_guard<std::mutex> g(a->gpu);
    return registry_to_device(a);
}

extern "C" nmn_status nmn_delta_set_to_device(nmn_delta_set* s) {
    if (!s) return set_error(NMN_ERR_INVALID_ARGUMENT, "null argument");
    std::shared_lock<std::shared_mutex> lk(s->reg->rw);
    std::lock_guard<std::mutex> g(s->reg->gpu);
    return mirrors(s);
}

extern "C" nmn_status nmn_archetypes_find_best_device(nmn_archetypes* a, const float* rows_dev, uint64_t n, int64_t* ids_dev, float* sims_dev,
                                                      void* stream) {
    if (!a || !rows_dev || !ids_dev || !sims_dev) return set_error(NMN_ERR_INVALID_ARGUMENT, "null argument");
    std::shared_lock<std::shared_mutex> lk(a->rw);
    if (a->len() == 0) return set_error(NMN_ERR_INVALID_ARGUMENT, "the registry is empty: find_best_archetype is None for every row");
    if (!a->d_valid || a->d_count != a->len())
        return set_error(NMN_ERR_INVALID_ARGUMENT, "the registry is not resident on the device: call nmn_archetypes_to_device after the last register");
    if (n == 0) return NMN_OK;
    if (a->device >= 0) D_TRY(hipSetDevice(a->device));
    launch_find_best(a, rows_dev, n, ids_dev, sims_dev, nullptr, static_cast<hipStream_t>(stream));
    D_TRY(hipGetLastError());
    return NMN_OK;
}

extern "C" nmn_status nmn_delta_set_dot_dense_device(nmn_delta_set* s, const float* queries_dev, uint32_t nq, float* scratch_dev, float* out_dev,
                                                     void* stream) {
    return score_device(s, queries_dev, nq, scratch_dev, out_dev, 0, stream);
}
extern "C" nmn_status nmn_delta_set_cosine_dense_device(nmn_delta_set* s, const float* queries_dev, uint32_t nq, float* scratch_dev,
                                                        float* out_dev, void* stream) {
    return score_device(s, queries_dev, nq, scratch_dev, out_dev, 1, stream);
}

// ---- top-k over a delta set (docs/delta.md §8) --------------------------------------------------------------------------------

extern "C" nmn_status nmn_deltaset_limits(uint32_t* select_chunk_rows, uint32_t* select_max_k, uint64_t* block_budget_bytes,
                                          uint64_t* sort_single_query_rows) {
    if (sort_single_query_rows) *sort_single_query_rows = kSortSingleRows;
    if (select_chunk_rows) *select_chunk_rows = kSelectChunk;
    if (select_max_k) *select_max_k = kSelectMaxK;
    if (block_budget_bytes) *block_budget_bytes = kSearchBudget;
    return NMN_OK;
}

extern "C" uint64_t nmn_deltaset_search_scratch_bytes(nmn_delta_set* s, uint32_t nq, uint32_t k) {
    if (!s) return 0;
    std::shared_lock<std::shared_mutex> lk(s->reg->rw);
    return SearchScratch(s->n, s->reg->len(), nq, k).bytes;
}

extern "C" nmn_status nmn_deltaset_search(nmn_delta_set* s, const float* queries, uint32_t nq, uint32_t k, int32_t cosine, uint64_t* rows_out,
                                          float* scores_out, uint32_t* counts_out) {
    return search(s, queries, nq, k, cosine != 0, rows_out, scores_out, counts_out);
}

extern "C" nmn_status nmn_deltaset_search_device(nmn_delta_set* s, const float* queries_dev, uint32_t nq, uint32_t k, int32_t cosine,
                                                 void* scratch_dev, uint64_t scratch_bytes, uint64_t* rows_dev, float* scores_dev,
                                                 uint32_t* counts_dev, void* stream) {
    return search_device(s, queries_dev, nq, k, cosine != 0, scratch_dev, scratch_bytes, rows_dev, scores_dev, counts_dev, stream);
}

// ---- sets made on the device (docs/delta.md §9) -------------------------------------------------------------------------------

extern "C" nmn_status nmn_deltaset_encode_device(nmn_archetypes* a, const float* rows_dev, uint64_t n, float threshold, int32_t with_magnitude,
                                                 int64_t* ids_dev, float* sims_dev, void* stream, nmn_delta_set** out) {
    if (!a || (!rows_dev && n) || !out) return set_error(NMN_ERR_INVALID_ARGUMENT, "null argument");
    *out = nullptr;
    std::shared_lock<std::shared_mutex> lk(a->rw);
    if (a->len() == 0) return set_error(NMN_ERR_INVALID_ARGUMENT, "the registry is empty: encode is None for every row");
    if (!a->d_valid || a->d_count != a->len())
        return set_error(NMN_ERR_INVALID_ARGUMENT, "the registry is not resident on the device: call nmn_archetypes_to_device after the last register");
    if (a->dim > NMN_DELTA_MAX_DIMENSION) return set_error(NMN_ERR_INVALID_ARGUMENT, dimension_exceeded(a->dim).c_str());
    nmn_delta_set* s = new nmn_delta_set();
    s->reg = a;
    s->indptr.assign(1, 0);
    if (n) {
        if (a->device >= 0) D_TRY(hipSetDevice(a->device));
        nmn_status st = encode_resident(a, nullptr, rows_dev, n, threshold, with_magnitude != 0, ids_dev, sims_dev, static_cast<hipStream_t>(stream), s);
        if (st != NMN_OK) {
            delete s;
            return st;
        }
    }
    *out = s;
    return NMN_OK;
}

extern "C" int32_t nmn_deltaset_host_arrays_present(nmn_delta_set* s) { return s && s->host_present.load(std::memory_order_acquire) ? 1 : 0; }
