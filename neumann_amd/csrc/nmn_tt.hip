// nmn_tt.hip — tensor-train vectors prepared on the GPU: tt_reconstruct (tensor_compress/src/tensor_train.rs:401-436) and tt_norm
// (440-474), bit for bit, for the TT queries of the HNSW walk (HNSWIndex::search_tt_with_ef, tensor_store/src/hnsw.rs:1811-1841)
// and for insert_tt_vector (1755-1759).  docs/hnsw.md §17.  Further down: tt_decompose (§21) and the comparisons of trains without
// reconstruction — tt_dot_product, tt_cosine_similarity, tt_euclidean_distance (480-546), §23.
// THIS TRANSLATION UNIT IS BUILT WITH -ffp-contract=off -fhip-fp32-correctly-rounded-divide-sqrt (build.py), host and device.
//
// Reference order restated here:
//   TTCore::get (tensor_train.rs:240-243): core k is r_k x n_k x r_{k+1} floats, element (i, j, r) at (i n_k + j) r_{k+1} + r.
//   tt_reconstruct: for every element, multi_idx from the flat index (the LAST mode runs fastest), then core by core
//       new[r] = (+0.0 + left[0] G[0,j,r]) + left[1] G[1,j,r] + ... — product and sum rounded separately, in l order, left = [1.0]
//       before the first core.  The chain of an element depends on its multi-index prefix only, so elements that share a prefix
//       share those values exactly: level k holds n_1 .. n_k vectors of length r_k, each computed once.
//   tt_norm: gram = [1.0]; per core, new_gram[a r2 + b] is ONE chain from +0.0 over k, then i, then j of
//       sum + ((gram[i r1 + j] * G[i,k,a]) * G[j,k,b]); at the end sqrt(gram[0]).
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <thread>
#include <vector>

#include "nmn_internal.h"
#include "nmn_tt.h"

#pragma clang fp contract(off)

namespace nmn {
namespace {

#define TT_TRY(expr)                                                  \
    do {                                                              \
        hipError_t _e = (expr);                                       \
        if (_e != hipSuccess) return set_error_hip(_e, #expr);        \
    } while (0)

struct TTArgs {
    uint32_t n_cores, nq, dim;
    uint32_t shape[kTTMaxCores];
    uint32_t ranks[kTTMaxCores + 1];  // qranks == nullptr: the one rank vector of the call
    const uint32_t* qranks;           // [nq][n_cores + 1]
    const uint64_t* core_off;         // [nq + 1], or null: query q starts at q * stride
    uint64_t stride;
    const float* cores;
    const uint8_t* skip;              // [nq] nullable: 1 = the host prepares this train
    float* rows;                      // [nq][dim] nullable
    float* norms;                     // [nq] nullable: tt_norm
    float* mags;                      // [nq] nullable: tt_norm, 0.0 where it is below 1e-10
};

// One workgroup per train, the trains beyond the grid in a stride loop.  The cores are staged in LDS once; then one pass per core
// computes the next reconstruction level (one thread per (prefix, r) output) and the next Gram matrix (one thread per (a, b)
// output), a barrier between passes.  No chain is split: every output is one thread's sequential f32 sum in the reference's order.
// The host has checked every size against the LDS arrays below (tt_check) — the kernel reads ranks the HOST supplied.
__global__ __launch_bounds__(256) void tt_prepare_kernel(TTArgs a) {
    __shared__ float s_core[kTTMaxStorage];
    __shared__ float s_lvl[2][kTTMaxLevel];
    __shared__ float s_gram[2][kTTMaxRank * kTTMaxRank];
    __shared__ uint32_t s_r[kTTMaxCores + 1];
    const uint32_t tid = threadIdx.x;
    const bool want_norm = a.norms || a.mags;
    for (uint32_t q = blockIdx.x; q < a.nq; q += gridDim.x) {
        if (a.skip && a.skip[q]) continue;  // (the same for every thread of the workgroup)
        __syncthreads();                    // the readers of the previous train are done
        if (tid <= a.n_cores) s_r[tid] = a.qranks ? a.qranks[(size_t)q * (a.n_cores + 1) + tid] : a.ranks[tid];
        __syncthreads();
        uint32_t storage = 0;
        for (uint32_t k = 0; k < a.n_cores; k++) storage += s_r[k] * a.shape[k] * s_r[k + 1];
        const float* src = a.cores + (a.core_off ? a.core_off[q] : (uint64_t)q * a.stride);
        for (uint32_t i = tid; i < storage; i += 256) s_core[i] = src[i];
        if (tid == 0) {
            s_lvl[0][0] = 1.0f;   // left_vec = [1.0]
            s_gram[0][0] = 1.0f;  // gram = [1.0]
        }
        __syncthreads();
        uint32_t prefix = 1, coff = 0;
        for (uint32_t k = 0; k < a.n_cores; k++) {
            const uint32_t r1 = s_r[k], n = a.shape[k], r2 = s_r[k + 1];
            const float* G = s_core + coff;
            const uint32_t cur = k & 1u, nxt = cur ^ 1u;
            if (a.rows) {
                const bool last = k + 1 == a.n_cores;  // r2 == 1: the outputs are the elements, in flat order
                const uint32_t total = prefix * n * r2;
                float* dst = last ? a.rows + (size_t)q * a.dim : s_lvl[nxt];
                for (uint32_t idx = tid; idx < total; idx += 256) {
                    const uint32_t pre = idx / r2, r = idx - pre * r2;
                    const uint32_t pp = pre / n, j = pre - pp * n;
                    const float* left = s_lvl[cur] + pp * r1;
                    float acc = 0.0f;
                    for (uint32_t l = 0; l < r1; l++) {
                        const float p = left[l] * G[(l * n + j) * r2 + r];
                        acc = acc + p;
                    }
                    dst[idx] = acc;
                }
            }
            if (want_norm) {
                const float* gram = s_gram[cur];
                for (uint32_t o = tid; o < r2 * r2; o += 256) {
                    const uint32_t ga = o / r2, gb = o - ga * r2;
                    float sum = 0.0f;
                    for (uint32_t kk = 0; kk < n; kk++)
                        for (uint32_t i = 0; i < r1; i++) {
                            const float gi = G[(i * n + kk) * r2 + ga];
                            for (uint32_t j = 0; j < r1; j++) {
                                const float t = gram[i * r1 + j] * gi;
                                const float p = t * G[(j * n + kk) * r2 + gb];
                                sum = sum + p;
                            }
                        }
                    s_gram[nxt][o] = sum;
                }
            }
            prefix *= n;
            coff += r1 * n * r2;
            __syncthreads();
        }
        if (want_norm && tid == 0) {
            const float nrm = __builtin_sqrtf(s_gram[a.n_cores & 1u][0]);
            if (a.norms) a.norms[q] = nrm;
            // The walk's cosine returns 1.0 when the query's magnitude == 0.0; cosine_distance_tt_with_norm returns 1.0 when
            // query_norm < 1e-10 (hnsw.rs:1199-1201).  A norm is a square root: never negative (-0.0 compares equal to 0.0), so
            // writing 0.0 for every norm below 1e-10 makes the two tests select exactly the same queries, and the value returned is
            // the same constant.  NaN < 1e-10 is false: a NaN norm stays NaN, as in the reference.
            if (a.mags) a.mags[q] = nrm < 1e-10f ? 0.0f : nrm;
        }
    }
}

bool host_forced() {
    const char* e = getenv("NMN_HNSW_HOST_SEARCH");
    return e && e[0] == '1';
}

nmn_status refuse(uint32_t q, const char* rule) {
    char buf[200];
    snprintf(buf, sizeof buf, "TT: query %u: %s", q, rule);
    return set_error(NMN_ERR_INVALID_ARGUMENT, buf);
}

}  // namespace

nmn_status tt_check(const uint32_t* shape, uint32_t n_cores, const uint32_t* ranks, bool per_query, const uint64_t* core_off,
                    uint32_t nq, bool host_env, TTBatch* b) {
    if (n_cores < 1 || n_cores > kTTMaxCores) return set_error(NMN_ERR_INVALID_ARGUMENT, "TT: n_cores must be 1..8");
    if (!shape || !ranks) return set_error(NMN_ERR_INVALID_ARGUMENT, "null argument");
    uint64_t dim = 1;
    for (uint32_t k = 0; k < n_cores; k++) {
        if (shape[k] < 1) return set_error(NMN_ERR_INVALID_ARGUMENT, "TT: every mode of the shape must be >= 1");
        dim *= shape[k];
        if (dim > (1ull << 31)) return set_error(NMN_ERR_INVALID_ARGUMENT, "TT: the product of the shape is above 2^31");
    }
    b->n_cores = n_cores;
    b->nq = nq;
    b->dim = dim;
    memcpy(b->shape, shape, n_cores * sizeof(uint32_t));
    b->ranks = ranks;
    b->per_query = per_query;
    b->core_off = core_off;
    b->on_host.assign(nq, 0);
    b->n_on_host = 0;
    const bool forced = host_env && host_forced();
    for (uint32_t q = 0; q < nq; q++) {
        const uint32_t* r = b->ranks_of(q);
        if (!per_query && q > 0) {  // one rank vector: checked once
            b->on_host[q] = b->on_host[0];
            b->n_on_host += b->on_host[q];
            continue;
        }
        if (r[0] != 1 || r[n_cores] != 1) return refuse(q, "ranks[0] and ranks[n_cores] must be 1");
        bool big = forced;
        uint64_t storage = 0, prefix = 1;
        for (uint32_t k = 0; k < n_cores; k++) {
            if (r[k + 1] < 1) return refuse(q, "every rank must be >= 1");
            if (r[k + 1] > (1u << 16)) return refuse(q, "a rank above 65536");
            storage += (uint64_t)r[k] * shape[k] * r[k + 1];
            if (storage > (1ull << 32)) return refuse(q, "core storage above 2^32 floats");
            prefix *= shape[k];
            if (r[k + 1] > kTTMaxRank) big = true;
            if (k + 1 < n_cores && prefix * r[k + 1] > kTTMaxLevel) big = true;
        }
        if (storage > kTTMaxStorage) big = true;
        if (core_off) {
            if (core_off[q + 1] < core_off[q]) return refuse(q, "core_off decreases");
            if (core_off[q + 1] - core_off[q] != storage)
                return refuse(q, "core_off[q + 1] - core_off[q] is not the sum of ranks[k] * shape[k] * ranks[k + 1]");
        }
        b->on_host[q] = big ? 1 : 0;
        b->n_on_host += b->on_host[q];
    }
    return NMN_OK;
}

void tt_reconstruct_host(const uint32_t* shape, uint32_t n_cores, const uint32_t* ranks, const float* cores, float* out) {
    std::vector<float> cur(1, 1.0f), nxt;
    uint64_t prefix = 1;
    const float* G = cores;
    for (uint32_t k = 0; k < n_cores; k++) {
        const uint64_t r1 = ranks[k], n = shape[k], r2 = ranks[k + 1];
        const bool last = k + 1 == n_cores;
        const uint64_t total = prefix * n * r2;
        if (!last) nxt.resize(total);
        float* dst = last ? out : nxt.data();
        for (uint64_t idx = 0; idx < total; idx++) {
            const uint64_t pre = idx / r2, r = idx - pre * r2;
            const uint64_t pp = pre / n, j = pre - pp * n;
            const float* left = cur.data() + pp * r1;
            float acc = 0.0f;
            for (uint64_t l = 0; l < r1; l++) {
                const float p = left[l] * G[(l * n + j) * r2 + r];
                acc = acc + p;
            }
            dst[idx] = acc;
        }
        if (!last) cur.swap(nxt);
        prefix *= n;
        G += r1 * n * r2;
    }
}

float tt_norm_host(const uint32_t* shape, uint32_t n_cores, const uint32_t* ranks, const float* cores) {
    std::vector<float> gram(1, 1.0f), ng;
    const float* G = cores;
    for (uint32_t k = 0; k < n_cores; k++) {
        const uint64_t r1 = ranks[k], n = shape[k], r2 = ranks[k + 1];
        ng.assign(r2 * r2, 0.0f);
        for (uint64_t ga = 0; ga < r2; ga++)
            for (uint64_t gb = 0; gb < r2; gb++) {
                float sum = 0.0f;
                for (uint64_t kk = 0; kk < n; kk++)
                    for (uint64_t i = 0; i < r1; i++)
                        for (uint64_t j = 0; j < r1; j++) {
                            const float t = gram[i * r1 + j] * G[(i * n + kk) * r2 + ga];
                            const float p = t * G[(j * n + kk) * r2 + gb];
                            sum = sum + p;
                        }
                ng[ga * r2 + gb] = sum;
            }
        gram.swap(ng);
        G += r1 * n * r2;
    }
    return sqrtf(gram[0]);
}

hipError_t launch_tt_prepare(const TTBatch& b, const float* cores_dev, const uint32_t* ranks_dev, const uint64_t* core_off_dev,
                             const uint8_t* skip_dev, float* rows_dev, float* norms_dev, float* mags_dev, hipStream_t s) {
    if (b.nq == 0 || b.n_on_host == b.nq) return hipSuccess;
    TTArgs a{};
    a.n_cores = b.n_cores;
    a.nq = b.nq;
    a.dim = (uint32_t)b.dim;
    memcpy(a.shape, b.shape, sizeof a.shape);
    if (!b.per_query) memcpy(a.ranks, b.ranks, (b.n_cores + 1) * sizeof(uint32_t));
    a.qranks = b.per_query ? ranks_dev : nullptr;
    a.core_off = b.core_off ? core_off_dev : nullptr;
    a.stride = b.core_off ? 0 : b.storage_of(0);
    a.cores = cores_dev;
    a.skip = b.n_on_host ? skip_dev : nullptr;
    a.rows = rows_dev;
    a.norms = norms_dev;
    a.mags = mags_dev;
    hipLaunchKernelGGL(tt_prepare_kernel, dim3(b.nq < kTTGridMax ? b.nq : kTTGridMax), dim3(256), 0, s, a);
    return hipGetLastError();
}

namespace {

// nmn_tt_reconstruct and nmn_tt_norm behind their argument checks: the trains within the LDS limits in one launch on the current
// device, the others by the host restatement
nmn_status tt_public(const uint32_t* shape, uint32_t n_cores, const uint32_t* ranks, const uint64_t* core_off, const float* cores,
                     uint32_t nq, float* out_rows, float* out_norms) {
    if (nq == 0) return NMN_OK;
    if (!core_off || (!out_rows && !out_norms)) return set_error(NMN_ERR_INVALID_ARGUMENT, "null argument");
    TTBatch b;
    nmn_status st = tt_check(shape, n_cores, ranks, true, core_off, nq, true, &b);
    if (st != NMN_OK) return st;
    if (core_off[nq] > core_off[0] && !cores) return set_error(NMN_ERR_INVALID_ARGUMENT, "null argument");
    b.cores = cores;
    const size_t dim = (size_t)b.dim;
    if (b.n_on_host < nq) {
        const uint64_t c0 = core_off[0], cn = core_off[nq] - c0;
        const size_t rk = (size_t)nq * (n_cores + 1);
        float *d_cores = nullptr, *d_rows = nullptr, *d_norms = nullptr;
        uint32_t* d_ranks = nullptr;
        uint64_t* d_off = nullptr;
        uint8_t* d_skip = nullptr;
        auto release = [&] {
            for (void* p : {(void*)d_cores, (void*)d_rows, (void*)d_norms, (void*)d_ranks, (void*)d_off, (void*)d_skip})
                if (p) (void)hipFree(p);
        };
        std::vector<uint64_t> off(core_off, core_off + nq + 1);
        for (uint64_t& o : off) o -= c0;
        auto body = [&]() -> nmn_status {
            TT_TRY(hipMalloc((void**)&d_cores, std::max<size_t>(cn * 4, 256)));
            TT_TRY(hipMalloc((void**)&d_ranks, rk * 4));
            TT_TRY(hipMalloc((void**)&d_off, (size_t)(nq + 1) * 8));
            TT_TRY(hipMalloc((void**)&d_skip, nq));
            if (out_rows) TT_TRY(hipMalloc((void**)&d_rows, (size_t)nq * dim * 4));
            if (out_norms) TT_TRY(hipMalloc((void**)&d_norms, (size_t)nq * 4));
            if (cn) TT_TRY(hipMemcpy(d_cores, cores + c0, cn * 4, hipMemcpyHostToDevice));
            TT_TRY(hipMemcpy(d_ranks, ranks, rk * 4, hipMemcpyHostToDevice));
            TT_TRY(hipMemcpy(d_off, off.data(), (size_t)(nq + 1) * 8, hipMemcpyHostToDevice));
            TT_TRY(hipMemcpy(d_skip, b.on_host.data(), nq, hipMemcpyHostToDevice));
            TT_TRY(launch_tt_prepare(b, d_cores, d_ranks, d_off, d_skip, d_rows, d_norms, nullptr, nullptr));
            TT_TRY(hipDeviceSynchronize());
            for (uint32_t q = 0; q < nq; q++) {  // (a row the host prepares is never read from the device's buffer)
                if (b.on_host[q]) continue;
                if (out_rows) TT_TRY(hipMemcpy(out_rows + (size_t)q * dim, d_rows + (size_t)q * dim, dim * 4, hipMemcpyDeviceToHost));
                if (out_norms) TT_TRY(hipMemcpy(out_norms + q, d_norms + q, 4, hipMemcpyDeviceToHost));
            }
            return NMN_OK;
        };
        st = body();
        release();
        if (st != NMN_OK) return st;
    }
    for (uint32_t q = 0; q < nq; q++) {
        if (!b.on_host[q]) continue;
        const uint32_t* r = b.ranks_of(q);
        if (out_rows) tt_reconstruct_host(shape, n_cores, r, cores + core_off[q], out_rows + (size_t)q * dim);
        if (out_norms) out_norms[q] = tt_norm_host(shape, n_cores, r, cores + core_off[q]);
    }
    return NMN_OK;
}

}  // namespace

// ---- tt_decompose (tensor_train.rs:315-397) -------------------------------------------------------------------------------------
//
// Reference order restated below, host and device (decompose.rs; docs/hnsw.md §21):
//   dot, frobenius_norm and the u = A v / v = A^T u sums of power_iteration are Iterator::sum::<f32>(): a left-to-right fold from
//       -0.0.  matmul's `let mut sum = 0.0` starts at +0.0.  Every product and every add is rounded on its own.
//   normalize: n = sqrt(dot(v, v)); x /= n (a true division) only when n > 1e-10f.
//   power_iteration: v_i = ((i * 7 + 3) % 13) as f32 / 13.0 - 0.5, normalised; at most 20 rounds of u = A v, normalize (its norm is
//       new_sigma), v = A^T u, normalize; |new_sigma - sigma| < 1e-6f * max(sigma, 1.0) returns new_sigma, the 20th round sigma.
//   svd_power_iteration: abs_tol = tolerance * frobenius_norm(A); per rank: sigma < abs_tol breaks (0 < 0 does not), otherwise
//       a[i][j] -= (sigma * u[i]) * v[j].
//   svd_truncated: rows > 32 && cols > 32 && 2 rank < min(rows, cols) takes the randomized path: Omega = gaussian_matrix(cols,
//       rank + min(5, min(rows, cols) - rank), rows * 31 + cols), Y = A Omega, Q = modified Gram-Schmidt of Y's columns (a column
//       whose norm is not above 1e-10f is dropped), B = Q^T A, the power-iteration SVD of B, U = Q U_B.
//   tt_decompose: core k = U (left n_k rows, new_rank columns), the next unfolding s[r] * vt[r][j]; the last core is what is left.
// NaN and infinite inputs are not refused and are outside the bit-level promise (max, the comparisons and libm differ there).

bool TTDecConfig::on_device() const {
    if (lds_floats > kTTDecMaxLdsFloats || dim > (1u << 20)) return false;
    for (uint32_t k = 0; k <= n_cores; k++)
        if (rb[k] > kTTDecMaxRank) return false;
    return true;
}

namespace {

struct RandomizedStep {
    bool taken;
    uint32_t rank, target;
};
// svd_truncated's choice (decompose.rs:407-418) for an unfolding of rows x cols
RandomizedStep randomized_step(uint64_t rows, uint64_t cols, uint64_t max_rank) {
    const uint64_t mn = std::min(rows, cols), rank = std::min(max_rank, mn);
    RandomizedStep r{rows > 32 && cols > 32 && rank * 2 < mn, (uint32_t)rank, 0};
    if (r.taken) r.target = (uint32_t)(rank + std::min<uint64_t>(5, mn - rank));
    return r;
}

struct TTDecLayout {  // offsets in floats into the dynamic LDS of tt_decompose_kernel
    uint32_t oA, oU, oV, oS, oUr, oUn, oVr, oVn, oB, oQ, oOm, total;
};

TTDecLayout dec_layout(const TTDecConfig& c) {
    uint64_t mA = 1, mU = 1, mV = 1, mRows = 1, mCols = 1, mRank = 1, mB = 0, mQ = 0, mOm = 0;
    uint64_t rem = c.dim;
    for (uint32_t k = 0; k + 1 < c.n_cores; k++) {
        rem /= c.shape[k];
        const uint64_t rows = (uint64_t)c.rb[k] * c.shape[k], cols = rem, ld = cols | 1;
        mA = std::max(mA, rows * ld);
        mU = std::max(mU, rows * c.rb[k + 1]);
        mV = std::max(mV, c.rb[k + 1] * cols);
        mRows = std::max(mRows, rows);
        mCols = std::max(mCols, cols);
        mRank = std::max<uint64_t>(mRank, c.rb[k + 1]);
        for (uint64_t l = 1; l <= c.rb[k]; l++) {
            const RandomizedStep r = randomized_step(l * c.shape[k], cols, c.max_rank);
            if (!r.taken) continue;
            mB = std::max(mB, r.target * ld);
            mQ = std::max(mQ, l * c.shape[k] * r.target);
            mOm = std::max(mOm, cols * r.target);
        }
    }
    const uint64_t sizes[11] = {mA, mU, mV, mRank, mRows, mRows, mCols, mCols, mB, mQ, mOm};
    uint32_t off[12];
    uint64_t at = 0;
    for (int i = 0; i < 11; i++) {
        off[i] = (uint32_t)std::min<uint64_t>(at, 1u << 30);
        at += sizes[i];
    }
    off[11] = (uint32_t)std::min<uint64_t>(at, 1u << 30);
    return {off[0], off[1], off[2], off[3], off[4], off[5], off[6], off[7], off[8], off[9], off[10], off[11]};
}

}  // namespace

nmn_status tt_dec_config(uint64_t dim, const uint32_t* shape, uint32_t n_cores, uint32_t max_rank, float tolerance, TTDecConfig* c,
                         char* debug, size_t debug_cap) {
    auto dbg = [&](const char* t) {
        if (debug && debug_cap) snprintf(debug, debug_cap, "%s", t);
    };
    if (dim == 0) {
        dbg("EmptyVector");
        return set_error(NMN_ERR_INVALID_ARGUMENT, "empty vector");
    }
    if (n_cores < 1 || n_cores > kTTMaxCores || !shape) {
        dbg("InvalidShape");
        return set_error(NMN_ERR_INVALID_ARGUMENT, "TT: n_cores must be 1..8");
    }
    unsigned __int128 product = 1;
    for (uint32_t k = 0; k < n_cores; k++) product = std::min<unsigned __int128>(product * shape[k], (unsigned __int128)1 << 100);
    if (product != dim) {
        char list[160], text[400];
        size_t at = 0;
        for (uint32_t k = 0; k < n_cores; k++)
            at += (size_t)snprintf(list + at, sizeof list - at, k ? ", %u" : "%u", shape[k]);
        const unsigned long long pr = product > ~0ull ? ~0ull : (unsigned long long)product;
        snprintf(text, sizeof text, "ShapeMismatch { dim: %llu, shape: [%s], product: %llu }", (unsigned long long)dim, list, pr);
        dbg(text);
        snprintf(text, sizeof text, "dimension %llu cannot be reshaped to [%s] (product: %llu)", (unsigned long long)dim, list, pr);
        return set_error(NMN_ERR_INVALID_ARGUMENT, text);
    }
    if (max_rank < 1) {
        dbg("InvalidRank");
        return set_error(NMN_ERR_INVALID_ARGUMENT, "invalid TT-rank: must be >= 1");
    }
    if (dim > (1ull << 31)) {
        dbg("InvalidShape");
        return set_error(NMN_ERR_INVALID_ARGUMENT, "TT: the product of the shape is above 2^31");
    }
    c->n_cores = n_cores;
    c->max_rank = max_rank;
    c->tolerance = tolerance;
    c->dim = dim;
    memcpy(c->shape, shape, n_cores * sizeof(uint32_t));
    c->rb[0] = 1;
    uint64_t rem = dim;
    for (uint32_t k = 0; k + 1 < n_cores; k++) {
        rem /= shape[k];
        c->rb[k + 1] = (uint32_t)std::min<uint64_t>(std::min<uint64_t>(max_rank, (uint64_t)c->rb[k] * shape[k]), rem);
    }
    c->rb[n_cores] = 1;
    c->slot = 0;
    for (uint32_t k = 0; k < n_cores; k++) c->slot += (uint64_t)c->rb[k] * shape[k] * c->rb[k + 1];
    c->lds_floats = dec_layout(*c).total;
    return NMN_OK;
}

namespace {

// ---- the host restatement ----

float normalize_host(float* v, size_t n) {
    float s = -0.0f;
    for (size_t i = 0; i < n; i++) {
        const float p = v[i] * v[i];
        s = s + p;
    }
    const float nr = sqrtf(s);
    if (nr > 1e-10f)
        for (size_t i = 0; i < n; i++) v[i] = v[i] / nr;
    return nr;
}

float power_iteration_host(const float* a, size_t rows, size_t cols, float* u, float* v) {
    for (size_t j = 0; j < cols; j++) v[j] = (float)((j * 7 + 3) % 13) / 13.0f - 0.5f;
    normalize_host(v, cols);
    float sigma = 0.0f;
    for (int it = 0; it < 20; it++) {
        for (size_t i = 0; i < rows; i++) {
            float s = -0.0f;
            for (size_t j = 0; j < cols; j++) {
                const float p = a[i * cols + j] * v[j];
                s = s + p;
            }
            u[i] = s;
        }
        const float new_sigma = normalize_host(u, rows);
        for (size_t j = 0; j < cols; j++) {
            float s = -0.0f;
            for (size_t i = 0; i < rows; i++) {
                const float p = a[i * cols + j] * u[i];
                s = s + p;
            }
            v[j] = s;
        }
        normalize_host(v, cols);
        const float bound = 1e-6f * (sigma > 1.0f ? sigma : 1.0f);
        if (fabsf(new_sigma - sigma) < bound) return new_sigma;
        sigma = new_sigma;
    }
    return sigma;
}

// svd_power_iteration of m (rows x cols, deflated in place): U [rows][rank] row-major, S, Vt [rank][cols]; returns the rank
size_t svd_power_host(float* m, size_t rows, size_t cols, size_t max_rank, float tolerance, std::vector<float>& U, std::vector<float>& S,
                      std::vector<float>& Vt) {
    const size_t rank = std::min(max_rank, std::min(rows, cols));
    float fs = -0.0f;
    for (size_t i = 0; i < rows * cols; i++) {
        const float p = m[i] * m[i];
        fs = fs + p;
    }
    const float abs_tol = tolerance * sqrtf(fs);
    std::vector<float> u(rows), v(cols), ucols;
    S.clear();
    Vt.clear();
    for (size_t c = 0; c < rank; c++) {
        const float sigma = power_iteration_host(m, rows, cols, u.data(), v.data());
        if (sigma < abs_tol) break;
        S.push_back(sigma);
        ucols.insert(ucols.end(), u.begin(), u.end());
        Vt.insert(Vt.end(), v.begin(), v.end());
        for (size_t i = 0; i < rows; i++) {
            const float su = sigma * u[i];
            for (size_t j = 0; j < cols; j++) {
                const float p = su * v[j];
                m[i * cols + j] = m[i * cols + j] - p;
            }
        }
    }
    const size_t got = S.size();
    U.assign(rows * got, 0.0f);
    for (size_t c = 0; c < got; c++)
        for (size_t i = 0; i < rows; i++) U[i * got + c] = ucols[c * rows + i];
    return got;
}

// gaussian_matrix (decompose.rs:271-294) with the platform's logf, cosf and sinf, which is what Rust's std calls
std::vector<float> gaussian_matrix_host(size_t rows, size_t cols, uint64_t seed) {
    uint64_t state = seed + 1;
    auto next = [&]() {
        state = state * 6364136223846793005ull + 1442695040888963407ull;
        return (float)(state >> 40) / 16777216.0f;
    };
    const size_t total = rows * cols;
    std::vector<float> data;
    data.reserve(total + 1);
    const float two_pi = 2.0f * 3.14159274101257324f;
    while (data.size() < total) {
        const float d1 = next();
        const float u1 = d1 > 1e-10f ? d1 : 1e-10f;
        const float u2 = next();
        const float r = sqrtf(-2.0f * ::logf(u1));
        const float theta = two_pi * u2;
        data.push_back(r * ::cosf(theta));
        if (data.size() < total) data.push_back(r * ::sinf(theta));
    }
    return data;
}

// c[i][j] = ((+0.0 + a[i][0] b[0][j]) + a[i][1] b[1][j]) + ..  (matmul, decompose.rs:197-216)
void matmul_host(const float* a, const float* b, size_t n, size_t inner, size_t m, float* c) {
    for (size_t i = 0; i < n; i++)
        for (size_t j = 0; j < m; j++) {
            float s = 0.0f;
            for (size_t k = 0; k < inner; k++) {
                const float p = a[i * inner + k] * b[k * m + j];
                s = s + p;
            }
            c[i * m + j] = s;
        }
}

size_t svd_truncated_host(std::vector<float>& m, size_t rows, size_t cols, size_t max_rank, float tolerance, std::vector<float>& U,
                          std::vector<float>& S, std::vector<float>& Vt) {
    const RandomizedStep rs = randomized_step(rows, cols, max_rank);
    if (!rs.taken) return svd_power_host(m.data(), rows, cols, max_rank, tolerance, U, S, Vt);
    const size_t t = rs.target;
    const std::vector<float> omega = gaussian_matrix_host(cols, t, (uint64_t)rows * 31 + cols);
    std::vector<float> y(rows * t);
    matmul_host(m.data(), omega.data(), rows, cols, t, y.data());
    std::vector<std::vector<float>> q;  // qr_orthonormalize: modified Gram-Schmidt over the columns
    std::vector<float> col(rows);
    for (size_t j = 0; j < t; j++) {
        for (size_t i = 0; i < rows; i++) col[i] = y[i * t + j];
        for (const std::vector<float>& qc : q) {
            float proj = -0.0f;
            for (size_t i = 0; i < rows; i++) {
                const float p = col[i] * qc[i];
                proj = proj + p;
            }
            for (size_t i = 0; i < rows; i++) {
                const float p = proj * qc[i];
                col[i] = col[i] - p;
            }
        }
        if (normalize_host(col.data(), rows) > 1e-10f) q.push_back(col);
    }
    S.clear();
    U.clear();
    Vt.clear();
    const size_t r = q.size();
    if (r == 0) return 0;
    std::vector<float> basis(rows * r), basis_t(r * rows), projected(r * cols), us;
    for (size_t c = 0; c < r; c++)
        for (size_t i = 0; i < rows; i++) basis[i * r + c] = basis_t[c * rows + i] = q[c][i];
    matmul_host(basis_t.data(), m.data(), r, rows, cols, projected.data());
    const size_t got = svd_power_host(projected.data(), r, cols, rs.rank, tolerance, us, S, Vt);
    if (got == 0) return 0;
    U.assign(rows * got, 0.0f);
    matmul_host(basis.data(), us.data(), rows, r, got, U.data());
    return got;
}

}  // namespace

uint32_t tt_decompose_host(const TTDecConfig& c, const float* vector, uint32_t* ranks_out, float* cores_out) {
    const uint32_t n = c.n_cores;
    std::vector<float> cur(vector, vector + c.dim), U, S, Vt;
    size_t left = 1, rem = c.dim, coff = 0;
    ranks_out[0] = 1;
    for (uint32_t k = 0; k + 1 < n; k++) {
        const size_t mode = c.shape[k], rows = left * mode;
        rem /= mode;
        if (cur.empty()) {  // a rank of 0 with another SVD to come: svd_truncated's EmptyMatrix
            for (uint32_t i = 0; i <= n; i++) ranks_out[i] = 0;
            return kTTStatusEmptyMatrix;
        }
        const size_t got = svd_truncated_host(cur, rows, rem, c.max_rank, c.tolerance, U, S, Vt);
        const size_t new_rank = std::min<size_t>(got, c.max_rank);
        ranks_out[k + 1] = (uint32_t)new_rank;
        if (cores_out)
            for (size_t row = 0; row < rows; row++)
                for (size_t r = 0; r < new_rank; r++) cores_out[coff + row * new_rank + r] = U[row * got + r];
        coff += rows * new_rank;
        cur.assign(new_rank * rem, 0.0f);
        for (size_t r = 0; r < new_rank; r++)
            for (size_t j = 0; j < rem; j++) cur[r * rem + j] = S[r] * Vt[r * rem + j];
        left = new_rank;
    }
    ranks_out[n] = 1;
    if (cores_out)
        for (size_t i = 0; i < cur.size(); i++) cores_out[coff + i] = cur[i];
    return kTTStatusOk;
}

void tt_decompose_host_batch(const TTDecConfig& c, const float* vectors, uint64_t n, uint32_t* status, uint32_t* ranks, float* cores,
                             unsigned threads) {
    auto work = [&](uint64_t lo, uint64_t hi) {
        for (uint64_t q = lo; q < hi; q++)
            status[q] = tt_decompose_host(c, vectors + q * c.dim, ranks + q * (c.n_cores + 1), cores ? cores + q * c.slot : nullptr);
    };
    threads = (unsigned)std::min<uint64_t>(std::max(threads, 1u), std::max<uint64_t>(n / 4, 1));
    if (threads <= 1) return work(0, n);
    std::vector<std::thread> pool;
    for (unsigned t = 0; t < threads; t++) pool.emplace_back(work, n * t / threads, n * (t + 1) / threads);
    for (std::thread& t : pool) t.join();
}

namespace {

uint32_t env_u32(const char* name, uint32_t dflt) {
    const char* e = getenv(name);
    if (!e || !*e) return dflt;
    char* end = nullptr;
    const unsigned long long v = strtoull(e, &end, 10);
    if (end == e) return dflt;
    return (uint32_t)std::min<unsigned long long>(v, 0xFFFFFFFFull);
}

}  // namespace

bool tt_decompose_on_host(const TTDecConfig& c, uint64_t n) {
    return host_forced() || !c.on_device() || n < env_u32("NMN_TT_DECOMPOSE_MIN", kTTDecMinDefault);
}

namespace {

// ---- the kernel ----

struct TTDecArgs {
    uint32_t n_cores, max_rank, dim;
    float tolerance;
    uint64_t n, slot;
    uint32_t shape[kTTMaxCores];
    const float* vectors;     // [n][dim]
    uint32_t* status;         // [n]
    uint32_t* ranks;          // [n][n_cores + 1]
    float* cores;             // nullable: status only
    uint64_t* core_off;       // nullable: [n + 1] = q * slot
    const uint32_t* om_off;   // [n_cores][kTTDecMaxRank + 1]: where the Gaussian matrix of step k with left rank l starts in om
    const float* om;
    TTDecLayout o;
};

// v / n where n = sqrt(dot(v, v)) > 1e-10f, v as it is otherwise: every thread folds the whole chain from LDS (broadcast reads),
// then the threads divide an element each.  raw is visible on entry, out on return.
__device__ float dec_normalize(const float* raw, float* out, uint32_t n) {
    float s = -0.0f;
    for (uint32_t i = 0; i < n; i++) {
        const float p = raw[i] * raw[i];
        s = s + p;
    }
    const float nr = __builtin_sqrtf(s);
    const bool divide = nr > 1e-10f;
    for (uint32_t i = threadIdx.x; i < n; i += blockDim.x) out[i] = divide ? raw[i] / nr : raw[i];
    __syncthreads();
    return nr;
}

// power_iteration of m (rows x cols, leading dimension ld): a thread per row of u and per column of v, each its own chain;
// returns sigma (the same value in every thread), u in un and v in vn
__device__ float dec_power_iteration(const float* m, uint32_t rows, uint32_t cols, uint32_t ld, float* ur, float* un, float* vr,
                                     float* vn) {
    const uint32_t tid = threadIdx.x, T = blockDim.x;
    for (uint32_t j = tid; j < cols; j += T) vr[j] = (float)((j * 7u + 3u) % 13u) / 13.0f - 0.5f;
    __syncthreads();
    dec_normalize(vr, vn, cols);
    float sigma = 0.0f;
    for (int it = 0; it < 20; it++) {
        for (uint32_t i = tid; i < rows; i += T) {
            const float* row = m + (size_t)i * ld;
            float s = -0.0f;
            for (uint32_t j = 0; j < cols; j++) {
                const float p = row[j] * vn[j];
                s = s + p;
            }
            ur[i] = s;
        }
        __syncthreads();
        const float new_sigma = dec_normalize(ur, un, rows);
        for (uint32_t j = tid; j < cols; j += T) {
            float s = -0.0f;
            for (uint32_t i = 0; i < rows; i++) {
                const float p = m[(size_t)i * ld + j] * un[i];
                s = s + p;
            }
            vr[j] = s;
        }
        __syncthreads();
        dec_normalize(vr, vn, cols);
        const float bound = 1e-6f * (sigma > 1.0f ? sigma : 1.0f);
        if (__builtin_fabsf(new_sigma - sigma) < bound) return new_sigma;
        sigma = new_sigma;
    }
    return sigma;
}

// svd_power_iteration of m, deflated in place: U column-major (column c at U + c * rows), V row-major [rank][cols], S; returns the
// rank.  m is visible on entry; U, V and S are visible on return.
__device__ uint32_t dec_svd_power(float* m, uint32_t rows, uint32_t cols, uint32_t ld, uint32_t max_rank, float tolerance, float* U,
                                  float* V, float* S, float* ur, float* un, float* vr, float* vn) {
    const uint32_t tid = threadIdx.x, T = blockDim.x;
    const uint32_t rank = min(max_rank, min(rows, cols));
    float fs = -0.0f;
    for (uint32_t i = 0; i < rows; i++)
        for (uint32_t j = 0; j < cols; j++) {
            const float x = m[(size_t)i * ld + j];
            const float p = x * x;
            fs = fs + p;
        }
    const float abs_tol = tolerance * __builtin_sqrtf(fs);
    uint32_t got = 0;
    for (uint32_t c = 0; c < rank; c++) {
        const float sigma = dec_power_iteration(m, rows, cols, ld, ur, un, vr, vn);
        if (sigma < abs_tol) break;
        for (uint32_t i = tid; i < rows; i += T) U[(size_t)got * rows + i] = un[i];
        for (uint32_t j = tid; j < cols; j += T) V[(size_t)got * cols + j] = vn[j];
        if (tid == 0) S[got] = sigma;
        for (uint32_t e = tid; e < rows * cols; e += T) {
            const uint32_t i = e / cols, j = e - i * cols;
            const float su = sigma * un[i];
            const float p = su * vn[j];
            m[(size_t)i * ld + j] = m[(size_t)i * ld + j] - p;
        }
        got++;
        __syncthreads();
    }
    return got;
}

// One workgroup owns one vector at a time, the vectors beyond the grid in a stride loop; the vector's whole state is in dynamic LDS
// (TTDecLayout).  No chain is split: the threads share out only the outputs the reference computes independently — the rows of u,
// the columns of v, the elements of a deflation, the outputs of a matmul, the elements of a Gram-Schmidt update — and the
// sequential norms and dots are folded by every thread from LDS.  Every branch below is taken by the whole workgroup.
__global__ __launch_bounds__(256) void tt_decompose_kernel(TTDecArgs a) {
    extern __shared__ float lds[];
    float *A = lds + a.o.oA, *U = lds + a.o.oU, *V = lds + a.o.oV, *S = lds + a.o.oS, *ur = lds + a.o.oUr, *un = lds + a.o.oUn,
          *vr = lds + a.o.oVr, *vn = lds + a.o.oVn, *B = lds + a.o.oB, *Q = lds + a.o.oQ, *Om = lds + a.o.oOm;
    const uint32_t tid = threadIdx.x, T = blockDim.x, n = a.n_cores;
    for (uint64_t q = blockIdx.x; q < a.n; q += gridDim.x) {
        const float* vec = a.vectors + q * a.dim;
        float* core = a.cores ? a.cores + q * a.slot : nullptr;
        uint32_t* rk = a.ranks + q * (n + 1);
        if (tid == 0 && a.core_off) {
            a.core_off[q] = q * a.slot;
            if (q + 1 == a.n) a.core_off[a.n] = a.n * a.slot;
        }
        __syncthreads();  // the readers of the previous vector are done
        uint32_t left = 1, rem = a.dim / a.shape[0], coff = 0;
        bool empty = false;
        if (n == 1) {
            if (core)
                for (uint32_t e = tid; e < a.dim; e += T) core[e] = vec[e];
        } else {
            const uint32_t ld0 = rem | 1u;
            for (uint32_t e = tid; e < a.dim; e += T) A[(size_t)(e / rem) * ld0 + e % rem] = vec[e];
        }
        if (tid == 0) rk[0] = 1;
        for (uint32_t k = 0; k + 1 < n; k++) {
            const uint32_t mode = a.shape[k], rows = left * mode, cols = rem, ld = cols | 1u;
            __syncthreads();
            const uint32_t mn = min(rows, cols), rank = min(a.max_rank, mn);
            const float* Uf = U;  // column-major, column c at Uf + c * rows
            uint32_t got;
            if (!(rows > 32 && cols > 32 && rank * 2 < mn)) {
                got = dec_svd_power(A, rows, cols, ld, a.max_rank, a.tolerance, U, V, S, ur, un, vr, vn);
            } else {
                const uint32_t t = rank + min(5u, mn - rank);
                const float* om = a.om + a.om_off[k * (kTTDecMaxRank + 1) + left];
                for (uint32_t e = tid; e < cols * t; e += T) Om[e] = om[e];
                __syncthreads();
                for (uint32_t e = tid; e < rows * t; e += T) {  // Y = A Omega, column-major into Q
                    const uint32_t c = e / rows, i = e - c * rows;
                    float s = 0.0f;
                    for (uint32_t kk = 0; kk < cols; kk++) {
                        const float p = A[(size_t)i * ld + kk] * Om[kk * t + c];
                        s = s + p;
                    }
                    Q[e] = s;
                }
                __syncthreads();
                uint32_t nq = 0;  // modified Gram-Schmidt, the kept columns packed to the front of Q
                for (uint32_t j = 0; j < t; j++) {
                    float* col = Q + (size_t)j * rows;
                    for (uint32_t pq = 0; pq < nq; pq++) {
                        const float* qc = Q + (size_t)pq * rows;
                        float proj = -0.0f;
                        for (uint32_t i = 0; i < rows; i++) {
                            const float p = col[i] * qc[i];
                            proj = proj + p;
                        }
                        __syncthreads();
                        for (uint32_t i = tid; i < rows; i += T) {
                            const float p = proj * qc[i];
                            col[i] = col[i] - p;
                        }
                        __syncthreads();
                    }
                    float s = -0.0f;
                    for (uint32_t i = 0; i < rows; i++) {
                        const float p = col[i] * col[i];
                        s = s + p;
                    }
                    const float nr = __builtin_sqrtf(s);
                    __syncthreads();
                    if (nr > 1e-10f) {
                        float* dst = Q + (size_t)nq * rows;
                        for (uint32_t i = tid; i < rows; i += T) dst[i] = col[i] / nr;
                        nq++;
                    }
                    __syncthreads();
                }
                got = 0;
                if (nq) {
                    for (uint32_t e = tid; e < nq * cols; e += T) {  // B = Q^T A
                        const uint32_t pq = e / cols, j = e - pq * cols;
                        float s = 0.0f;
                        for (uint32_t kk = 0; kk < rows; kk++) {
                            const float p = Q[(size_t)pq * rows + kk] * A[(size_t)kk * ld + j];
                            s = s + p;
                        }
                        B[(size_t)pq * ld + j] = s;
                    }
                    __syncthreads();
                    got = dec_svd_power(B, nq, cols, ld, rank, a.tolerance, U, V, S, ur, un, vr, vn);
                    for (uint32_t e = tid; e < rows * got; e += T) {  // U = Q U_B, into A: the unfolding is dead
                        const uint32_t c = e / rows, i = e - c * rows;
                        float s = 0.0f;
                        for (uint32_t kk = 0; kk < nq; kk++) {
                            const float p = Q[(size_t)kk * rows + i] * U[(size_t)c * nq + kk];
                            s = s + p;
                        }
                        A[e] = s;
                    }
                    __syncthreads();
                    Uf = A;
                }
            }
            const uint32_t new_rank = min(got, a.max_rank);
            if (tid == 0) rk[k + 1] = new_rank;
            if (new_rank == 0 && k + 2 < n) {  // the next unfolding is empty: svd_truncated's EmptyMatrix
                empty = true;
                break;
            }
            if (core)
                for (uint32_t e = tid; e < rows * new_rank; e += T) {
                    const uint32_t row = e / new_rank, r = e - row * new_rank;
                    core[coff + e] = Uf[(size_t)r * rows + row];
                }
            coff += rows * new_rank;
            const uint32_t total = new_rank * cols;
            if (k + 2 == n) {  // what is left is the last core
                if (core)
                    for (uint32_t e = tid; e < total; e += T) core[coff + e] = S[e / cols] * V[e];
            } else {
                const uint32_t ncols = cols / a.shape[k + 1], nld = ncols | 1u;
                __syncthreads();  // Uf may be in A
                for (uint32_t e = tid; e < total; e += T) A[(size_t)(e / ncols) * nld + e % ncols] = S[e / cols] * V[e];
            }
            left = new_rank;
            rem = cols / a.shape[k + 1];
        }
        if (tid == 0) {
            if (empty) {
                for (uint32_t i = 0; i <= n; i++) rk[i] = 0;
            } else {
                rk[n] = 1;
            }
            a.status[q] = empty ? kTTStatusEmptyMatrix : kTTStatusOk;
        }
    }
}

// The Gaussian matrices of one config, made on the host (logf, cosf and sinf are the host libm's, as in the reference) and kept on
// the device for the life of the process: [n_cores][kTTDecMaxRank + 1] offsets, then the matrices.
struct DevOmega {
    int device;
    uint32_t n_cores, max_rank, shape[kTTMaxCores];
    uint32_t* off;
    float* data;
};
std::mutex g_omega_mu;
std::vector<DevOmega> g_omega;

nmn_status omega_for(const TTDecConfig& c, const DevOmega** out) {
    int dev = 0;
    TT_TRY(hipGetDevice(&dev));
    std::lock_guard<std::mutex> lk(g_omega_mu);
    for (const DevOmega& o : g_omega)
        if (o.device == dev && o.n_cores == c.n_cores && o.max_rank == c.max_rank && !memcmp(o.shape, c.shape, sizeof o.shape)) {
            *out = &o;
            return NMN_OK;
        }
    const size_t table = (size_t)c.n_cores * (kTTDecMaxRank + 1);
    std::vector<uint32_t> off(table, 0);
    std::vector<float> data(1, 0.0f);
    uint64_t rem = c.dim;
    for (uint32_t k = 0; k + 1 < c.n_cores; k++) {
        rem /= c.shape[k];
        for (uint32_t l = 1; l <= c.rb[k]; l++) {
            const uint64_t rows = (uint64_t)l * c.shape[k];
            const RandomizedStep r = randomized_step(rows, rem, c.max_rank);
            if (!r.taken) continue;
            const std::vector<float> g = gaussian_matrix_host(rem, r.target, rows * 31 + rem);
            off[k * (kTTDecMaxRank + 1) + l] = (uint32_t)data.size();
            data.insert(data.end(), g.begin(), g.end());
        }
    }
    DevOmega o{};
    o.device = dev;
    o.n_cores = c.n_cores;
    o.max_rank = c.max_rank;
    memcpy(o.shape, c.shape, sizeof o.shape);
    TT_TRY(hipMalloc((void**)&o.off, table * 4));
    if (hipError_t e = hipMalloc((void**)&o.data, data.size() * 4); e != hipSuccess) {
        (void)hipFree(o.off);
        return set_error_hip(e, "hipMalloc");
    }
    hipError_t e = hipMemcpy(o.off, off.data(), table * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(o.data, data.data(), data.size() * 4, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        (void)hipFree(o.off);
        (void)hipFree(o.data);
        return set_error_hip(e, "hipMemcpy");
    }
    g_omega.reserve(64);
    g_omega.push_back(o);
    *out = &g_omega.back();
    return NMN_OK;
}

}  // namespace

nmn_status launch_tt_decompose(const TTDecConfig& c, const float* vectors_dev, uint64_t n, uint32_t* status_dev, uint32_t* ranks_dev,
                               float* cores_dev, uint64_t* core_off_dev, hipStream_t s) {
    if (n == 0) return NMN_OK;
    if (!c.on_device()) return set_error(NMN_ERR_INVALID_ARGUMENT, "TT: the config is above the limits of the device's tt_decompose");
    const DevOmega* om = nullptr;
    nmn_status st = omega_for(c, &om);
    if (st != NMN_OK) return st;
    TTDecArgs a{};
    a.n_cores = c.n_cores;
    a.max_rank = c.max_rank;
    a.dim = (uint32_t)c.dim;
    a.tolerance = c.tolerance;
    a.n = n;
    a.slot = c.slot;
    memcpy(a.shape, c.shape, sizeof a.shape);
    a.vectors = vectors_dev;
    a.status = status_dev;
    a.ranks = ranks_dev;
    a.cores = cores_dev;
    a.core_off = core_off_dev;
    a.om_off = om->off;
    a.om = om->data;
    a.o = dec_layout(c);
    uint32_t threads = env_u32("NMN_TT_DECOMPOSE_THREADS", kTTDecThreads);
    if (threads != 64 && threads != 128 && threads != 256) threads = kTTDecThreads;
    const uint32_t grid_max = std::max(env_u32("NMN_TT_DECOMPOSE_GRID", kTTDecGridMax), 1u);
    hipLaunchKernelGGL(tt_decompose_kernel, dim3((uint32_t)std::min<uint64_t>(n, grid_max)), dim3(threads), a.o.total * sizeof(float), s, a);
    TT_TRY(hipGetLastError());
    return NMN_OK;
}

// ---- tt_dot_product, tt_cosine_similarity, tt_euclidean_distance (tensor_train.rs:480-546) ---------------------------------------
//
// Reference order restated below, host and device (docs/hnsw.md §23):
//   tt_dot_product(a, b): gram = [1.0]; per pair of cores (r1a, n, r2a) and (r1b, n, r2b), new_gram[x r2b + y] is ONE chain from
//       +0.0 over k, then ia, then ib of sum + ((gram[ia r1b + ib] * A[ia,k,x]) * B[ib,k,y]); the result is gram[0].  With a == b it
//       is the chain tt_norm runs before its square root.
//   tt_cosine_similarity: 0.0 when sqrt(dot(a,a)) or sqrt(dot(b,b)) is < 1e-10f (a NaN is not), else dot / (norm_a * norm_b).
//   tt_euclidean_distance: sqrt(max(fma(-2, dot_ab, dot_aa + dot_bb), 0.0)), the fma fused; f32::max drops a NaN: NaN gives 0.0.

float tt_dot_host(const uint32_t* shape, uint32_t n_cores, const uint32_t* ranks_a, const float* cores_a, const uint32_t* ranks_b,
                  const float* cores_b) {
    std::vector<float> gram(1, 1.0f), ng;
    const float *A = cores_a, *B = cores_b;
    for (uint32_t k = 0; k < n_cores; k++) {
        const uint64_t r1a = ranks_a[k], r2a = ranks_a[k + 1], r1b = ranks_b[k], r2b = ranks_b[k + 1], n = shape[k];
        ng.assign(r2a * r2b, 0.0f);
        for (uint64_t x = 0; x < r2a; x++)
            for (uint64_t y = 0; y < r2b; y++) {
                float sum = 0.0f;
                for (uint64_t kk = 0; kk < n; kk++)
                    for (uint64_t ia = 0; ia < r1a; ia++)
                        for (uint64_t ib = 0; ib < r1b; ib++) {
                            const float t = gram[ia * r1b + ib] * A[(ia * n + kk) * r2a + x];
                            const float p = t * B[(ib * n + kk) * r2b + y];
                            sum = sum + p;
                        }
                ng[x * r2b + y] = sum;
            }
        gram.swap(ng);
        A += r1a * n * r2a;
        B += r1b * n * r2b;
    }
    return gram[0];
}

namespace {

// what the three functions make of dot(a, b), dot(a, a) and dot(b, b)
__host__ __device__ inline float tt_sim_finish(uint32_t op, float dot, float self_a, float self_b) {
    if (op == NMN_TT_SIM_DOT) return dot;
    if (op == NMN_TT_SIM_COSINE) {
        const float na = __builtin_sqrtf(self_a), nb = __builtin_sqrtf(self_b);
        if (na < 1e-10f || nb < 1e-10f) return 0.0f;
        const float d = na * nb;
        return dot / d;
    }
    const float s = self_a + self_b;
    const float sq = __builtin_fmaf(-2.0f, dot, s);
    return __builtin_sqrtf(sq > 0.0f ? sq : 0.0f);  // max(sq, 0.0): a NaN and every value <= 0 give +0.0 (sq is never -0.0)
}

struct TTSet {  // one set of trains in DEVICE memory
    const uint32_t* ranks;     // [n][n_cores + 1]
    const uint64_t* core_off;  // nullable: train i starts at i * stride
    const float* cores;        // cap floats
    const uint32_t* status;    // nullable: a train whose status is not NMN_TT_OK is bad
    const uint8_t* skip;       // nullable: 1 = the host computes what this train takes part in
    uint64_t stride, cap;
    uint32_t n, max_rank;      // no rank of a good train is above max_rank (kTTMaxRank at most)
};

struct TTSimArgs {
    uint32_t op, n_cores;
    uint32_t shape[kTTMaxCores];
    TTSet q, t;
    const float *self_q, *self_t;  // null for NMN_TT_SIM_DOT
    float* out;                    // [nq][nt]; tt_self_dot_kernel: [t.n]
    uint32_t chunk, n_chunks;      // targets per work item (a multiple of the workgroup's waves), chunks per query
    uint32_t qcap, gcap;           // LDS floats for the query's cores, and for ONE Gram matrix of one wave
};

constexpr uint32_t kTTBadBits = 0x7FC00000u;  // what a bad train leaves in every output it takes part in

// The ranks of train i come from device memory: nothing is read through them before this has passed.  Bad: a status that is not
// NMN_TT_OK, end ranks that are not 1, a rank of 0 or above the set's max_rank, more core floats than `lim` (the slot, at most
// kTTMaxStorage), or core data that would leave the `cap` floats of the set's buffer.  *off: where the train's cores start.
__device__ bool tt_train_ok(const TTSet& s, uint32_t i, uint32_t n_cores, const uint32_t* shape, uint64_t lim, uint64_t* off) {
    const uint32_t* r = s.ranks + (size_t)i * (n_cores + 1);
    bool ok = !s.status || s.status[i] == kTTStatusOk;
    uint32_t r1 = r[0];
    ok = ok && r1 == 1;
    uint64_t storage = 0;
    for (uint32_t k = 0; k < n_cores; k++) {
        const uint32_t r2 = r[k + 1];
        ok = ok && r2 >= 1 && r2 <= s.max_rank;
        if (ok) storage += (uint64_t)r1 * shape[k] * r2;  // (r1, r2 <= 32 here: no overflow)
        ok = ok && storage <= lim;
        r1 = r2;
    }
    ok = ok && r1 == 1;
    uint64_t o = (uint64_t)i * s.stride;
    if (s.core_off) {
        const uint64_t lo = s.core_off[i], hi = s.core_off[i + 1];
        ok = ok && hi >= lo && storage <= hi - lo;
        o = lo;
    }
    ok = ok && o <= s.cap && storage <= s.cap - o;
    *off = o;
    return ok;
}

// (tt_gram_step, one core step of one pair by one wave, is nmn_tt.h's: the HNSW walk restates tt_dot_product with the same text)

// Dynamic LDS of both kernels, in floats: [qcap] the query's cores (tt_similarity_kernel only), then per wave two Gram matrices of
// gcap floats and the wave's train's ranks.
constexpr uint32_t kTTSimRankSlots = kTTMaxCores + 1;

// One workgroup takes one work item at a time — a query and a chunk of the targets — the items beyond the grid in a stride loop.
// The query's cores are staged in LDS once per item; then every wave owns one target at a time and walks the cores of its pair,
// the target's cores read from global memory.  No chain is split.  Every barrier is reached by the whole workgroup: the trips of
// the target loop and the core loop do not depend on the wave.
__global__ __launch_bounds__(256) void tt_similarity_kernel(TTSimArgs a) {
    extern __shared__ float lds[];
    __shared__ uint32_t s_ra[kTTSimRankSlots];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6, waves = blockDim.x >> 6;
    float* s_core = lds;
    float* s_gram = lds + a.qcap + (size_t)wave * (2 * a.gcap + kTTSimRankSlots);
    uint32_t* s_rb = (uint32_t*)(s_gram + 2 * a.gcap);
    const uint32_t n = a.n_cores, nt = a.t.n;
    const uint64_t lim_q = a.q.stride < a.qcap ? a.q.stride : a.qcap;
    const uint64_t lim_t = a.t.stride < kTTMaxStorage ? a.t.stride : kTTMaxStorage;
    const float bad = __uint_as_float(kTTBadBits);
    const uint64_t items = (uint64_t)a.q.n * a.n_chunks;
    for (uint64_t item = blockIdx.x; item < items; item += gridDim.x) {
        const uint32_t q = (uint32_t)(item / a.n_chunks), t0 = (uint32_t)(item - (uint64_t)q * a.n_chunks) * a.chunk;
        if (a.q.skip && a.q.skip[q]) continue;  // (the same for every thread of the workgroup)
        const uint32_t t_end = nt - t0 < a.chunk ? nt : t0 + a.chunk;
        uint64_t off_q;
        const bool ok_q = tt_train_ok(a.q, q, n, a.shape, lim_q, &off_q);
        __syncthreads();  // the readers of the previous item are done
        if (ok_q) {
            if (tid <= n) s_ra[tid] = a.q.ranks[(size_t)q * (n + 1) + tid];
            __syncthreads();
            uint32_t storage = 0;
            for (uint32_t k = 0; k < n; k++) storage += s_ra[k] * a.shape[k] * s_ra[k + 1];
            const float* src = a.q.cores + off_q;
            for (uint32_t i = tid; i < storage; i += blockDim.x) s_core[i] = src[i];
        }
        const float self_q = a.self_q && ok_q ? a.self_q[q] : 0.0f;
        for (uint32_t tb = t0; tb < t_end; tb += waves) {
            const uint32_t t = tb + wave;
            const bool mine = t < t_end && !(a.t.skip && a.t.skip[t]);
            uint64_t off_t = 0;
            const bool ok = mine && ok_q && tt_train_ok(a.t, t, n, a.shape, lim_t, &off_t);
            if (ok) {
                if (lane <= n) s_rb[lane] = a.t.ranks[(size_t)t * (n + 1) + lane];
                if (lane == 0) s_gram[0] = 1.0f;  // gram = [1.0]
            }
            uint32_t ca = 0, cb = 0;
            for (uint32_t k = 0; k < n; k++) {
                __syncthreads();
                if (ok) {
                    const uint32_t r1a = s_ra[k], r2a = s_ra[k + 1], r1b = s_rb[k], r2b = s_rb[k + 1], m = a.shape[k];
                    const uint32_t cur = k & 1u;
                    tt_gram_step(s_core + ca, a.t.cores + off_t + cb, s_gram + cur * a.gcap, s_gram + (cur ^ 1u) * a.gcap, r1a, r2a, r1b,
                                 r2b, m, lane);
                    ca += r1a * m * r2a;
                    cb += r1b * m * r2b;
                }
            }
            __syncthreads();
            if (mine && lane == 0) {
                float v = bad;
                if (ok) v = tt_sim_finish(a.op, s_gram[(n & 1u) * a.gcap], self_q, a.self_t ? a.self_t[t] : 0.0f);
                a.out[(size_t)q * nt + t] = v;
            }
            __syncthreads();  // the wave's ranks and gram[0] are free for the next target
        }
    }
}

// out[i] = tt_dot_product(t_i, t_i): a wave per train, groups of the workgroup's waves in a stride loop, both operands read from
// global memory.  A bad train's self dot is the quiet NaN.
__global__ __launch_bounds__(256) void tt_self_dot_kernel(TTSimArgs a) {
    extern __shared__ float lds[];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6, waves = blockDim.x >> 6;
    float* s_gram = lds + (size_t)wave * (2 * a.gcap + kTTSimRankSlots);
    uint32_t* s_r = (uint32_t*)(s_gram + 2 * a.gcap);
    const uint32_t n = a.n_cores, nt = a.t.n;
    const uint64_t lim = a.t.stride < kTTMaxStorage ? a.t.stride : kTTMaxStorage;
    for (uint64_t tb = (uint64_t)blockIdx.x * waves; tb < nt; tb += (uint64_t)gridDim.x * waves) {
        const uint32_t t = (uint32_t)tb + wave;
        const bool mine = t < nt && !(a.t.skip && a.t.skip[t]);
        uint64_t off = 0;
        const bool ok = mine && tt_train_ok(a.t, t, n, a.shape, lim, &off);
        if (ok) {
            if (lane <= n) s_r[lane] = a.t.ranks[(size_t)t * (n + 1) + lane];
            if (lane == 0) s_gram[0] = 1.0f;
        }
        uint32_t c = 0;
        for (uint32_t k = 0; k < n; k++) {
            __syncthreads();
            if (ok) {
                const uint32_t r1 = s_r[k], r2 = s_r[k + 1], m = a.shape[k], cur = k & 1u;
                const float* G = a.t.cores + off + c;
                tt_gram_step(G, G, s_gram + cur * a.gcap, s_gram + (cur ^ 1u) * a.gcap, r1, r2, r1, r2, m, lane);
                c += r1 * m * r2;
            }
        }
        __syncthreads();
        if (mine && lane == 0) a.out[t] = ok ? s_gram[(n & 1u) * a.gcap] : __uint_as_float(kTTBadBits);
        __syncthreads();
    }
}

// The workgroup shape of one launch: as many waves (4 at most) as the LDS of one workgroup holds Gram pairs beside the query's cores
struct TTSimShape {
    uint32_t waves, lds_bytes;
};
TTSimShape sim_shape(uint32_t qcap, uint32_t gcap) {
    const uint32_t per_wave = 2 * gcap + kTTSimRankSlots;
    const uint32_t waves = std::min<uint32_t>(4, (kTTSimMaxLdsFloats - qcap) / per_wave);
    return {waves, (qcap + waves * per_wave) * (uint32_t)sizeof(float)};
}

uint32_t sim_grid_max() { return std::max(env_u32("NMN_TT_SIMILARITY_GRID", kTTSimGridMax), 1u); }

void fill_set(TTSet* s, const TTSimSet& in) {
    s->ranks = in.ranks_dev;
    s->core_off = in.core_off_dev;
    s->cores = in.cores_dev;
    s->status = in.status_dev;
    s->skip = in.skip_dev;
    s->stride = in.stride;
    s->cap = in.cap;
    s->n = in.n;
    s->max_rank = std::min(std::max(in.max_rank, 1u), kTTMaxRank);
}

}  // namespace

hipError_t launch_tt_self_dot(const uint32_t* shape, uint32_t n_cores, const TTSimSet& set, float* out_dev, hipStream_t s) {
    if (set.n == 0) return hipSuccess;
    TTSimArgs a{};
    a.n_cores = n_cores;
    memcpy(a.shape, shape, n_cores * sizeof(uint32_t));
    fill_set(&a.t, set);
    a.out = out_dev;
    a.gcap = a.t.max_rank * a.t.max_rank;
    const TTSimShape ws = sim_shape(0, a.gcap);
    const uint32_t groups = (set.n + ws.waves - 1) / ws.waves;
    hipLaunchKernelGGL(tt_self_dot_kernel, dim3(std::min(groups, sim_grid_max())), dim3(ws.waves * 64), ws.lds_bytes, s, a);
    return hipGetLastError();
}

hipError_t launch_tt_similarity(uint32_t op, const uint32_t* shape, uint32_t n_cores, const TTSimSet& q, const TTSimSet& t,
                                const float* self_q_dev, const float* self_t_dev, float* out_dev, hipStream_t s) {
    if (q.n == 0 || t.n == 0) return hipSuccess;
    TTSimArgs a{};
    a.op = op;
    a.n_cores = n_cores;
    memcpy(a.shape, shape, n_cores * sizeof(uint32_t));
    fill_set(&a.q, q);
    fill_set(&a.t, t);
    a.self_q = op == NMN_TT_SIM_DOT ? nullptr : self_q_dev;
    a.self_t = op == NMN_TT_SIM_DOT ? nullptr : self_t_dev;
    a.out = out_dev;
    a.qcap = (uint32_t)std::min<uint64_t>(q.stride, kTTMaxStorage);
    a.gcap = a.q.max_rank * a.t.max_rank;
    const TTSimShape ws = sim_shape(a.qcap, a.gcap);
    // about grid_max work items: every query's targets in chunks of a multiple of the waves
    const uint32_t grid_max = sim_grid_max();
    const uint32_t per_query = std::max(grid_max / q.n, 1u);
    const uint64_t chunk = ((uint64_t)(t.n + per_query - 1) / per_query + ws.waves - 1) / ws.waves * ws.waves;
    a.chunk = (uint32_t)std::min<uint64_t>(chunk, 0xFFFFFF00u);
    a.n_chunks = (uint32_t)(((uint64_t)t.n + a.chunk - 1) / a.chunk);
    const uint64_t items = (uint64_t)q.n * a.n_chunks;
    hipLaunchKernelGGL(tt_similarity_kernel, dim3((uint32_t)std::min<uint64_t>(items, grid_max)), dim3(ws.waves * 64), ws.lds_bytes, s, a);
    return hipGetLastError();
}

namespace {

// TTConfig::for_dim's shape (tensor_train.rs:130-199): the table, then factorize_balanced with the host libm's f64 log2 and pow
std::vector<uint32_t> optimal_shape(uint64_t dim) {
    switch (dim) {
        case 64: return {4, 4, 4};
        case 128: return {4, 4, 8};
        case 256: return {4, 8, 8};
        case 384: return {4, 8, 12};
        case 512: return {8, 8, 8};
        case 768: return {8, 8, 12};
        case 1024: return {8, 8, 16};
        case 1536: return {8, 12, 16};
        case 2048: return {8, 16, 16};
        case 3072: return {8, 16, 24};
        case 4096: return {8, 8, 8, 8};
        case 8192: return {8, 8, 8, 16};
    }
    if (dim == 1) return {1};
    const double log_n = ceil(log2((double)dim));
    const uint64_t target_factors = std::min<uint64_t>(std::max<uint64_t>((uint64_t)log_n, 2), 6);
    const uint64_t target_size = (uint64_t)pow((double)dim, 1.0 / (double)target_factors);
    std::vector<uint32_t> factors;
    uint64_t remaining = dim;
    for (uint64_t it = 0; it + 1 < target_factors; it++) {
        uint64_t best = 1;
        for (uint64_t f = std::max<uint64_t>(target_size, 2); f >= 2; f--)
            if (remaining % f == 0) {
                best = f;
                break;
            }
        if (best == 1) {
            for (uint64_t f = 2; f * f <= remaining; f++)  // (the smallest factor; a prime's is itself)
                if (remaining % f == 0) {
                    best = f;
                    break;
                }
            if (best == 1) best = remaining;
        }
        factors.push_back((uint32_t)best);
        remaining /= best;
        if (remaining == 1) break;
    }
    if (remaining > 1) factors.push_back((uint32_t)remaining);
    std::sort(factors.begin(), factors.end());
    return factors;
}

}  // namespace
}  // namespace nmn

extern "C" nmn_status nmn_tt_config_for_dim(uint64_t dim, uint32_t preset, uint32_t* shape_out, uint32_t* n_cores_out,
                                            uint32_t* max_rank_out, float* tolerance_out) {
    if (dim == 0) return nmn::set_error(NMN_ERR_INVALID_ARGUMENT, "empty vector");
    if (dim > 0xFFFFFFFFull) return nmn::set_error(NMN_ERR_INVALID_ARGUMENT, "TT: dim above 2^32");
    if (preset > NMN_TT_PRESET_HIGH_ACCURACY) return nmn::set_error(NMN_ERR_INVALID_ARGUMENT, "TT: unknown preset");
    if (!shape_out || !n_cores_out) return nmn::set_error(NMN_ERR_INVALID_ARGUMENT, "null argument");
    const std::vector<uint32_t> shape = nmn::optimal_shape(dim);
    for (size_t k = 0; k < shape.size(); k++) shape_out[k] = shape[k];
    *n_cores_out = (uint32_t)shape.size();
    static const uint32_t rank[3] = {8, 4, 16};
    static const float tol[3] = {1e-4f, 1e-2f, 1e-6f};
    if (max_rank_out) *max_rank_out = rank[preset];
    if (tolerance_out) *tolerance_out = tol[preset];
    return NMN_OK;
}

extern "C" uint64_t nmn_tt_max_storage(const uint32_t* shape, uint32_t n_cores, uint32_t max_rank) {
    if (!shape || n_cores < 1 || n_cores > nmn::kTTMaxCores || max_rank < 1) return 0;
    unsigned __int128 dim = 1;
    for (uint32_t k = 0; k < n_cores; k++) dim *= shape[k];
    if (dim == 0 || dim > (1ull << 31)) return 0;
    nmn::TTDecConfig c;
    if (nmn::tt_dec_config((uint64_t)dim, shape, n_cores, max_rank, 1e-4f, &c, nullptr, 0) != NMN_OK) return 0;
    return c.slot;
}

extern "C" nmn_status nmn_tt_decompose_limits(uint32_t* max_cores, uint32_t* max_rank, uint32_t* max_dim, uint32_t* max_lds_floats) {
    if (max_cores) *max_cores = nmn::kTTMaxCores;
    if (max_rank) *max_rank = nmn::kTTDecMaxRank;
    if (max_dim) *max_dim = nmn::kTTDecMaxLdsFloats - 1;  // the first unfolding alone, padded, must fit
    if (max_lds_floats) *max_lds_floats = nmn::kTTDecMaxLdsFloats;
    return NMN_OK;
}

extern "C" uint64_t nmn_tt_decompose_lds_floats(const uint32_t* shape, uint32_t n_cores, uint32_t max_rank) {
    if (!shape || n_cores < 1 || n_cores > nmn::kTTMaxCores || max_rank < 1) return 0;
    unsigned __int128 dim = 1;
    for (uint32_t k = 0; k < n_cores; k++) dim *= shape[k];
    if (dim == 0 || dim > (1ull << 31)) return 0;
    nmn::TTDecConfig c;
    if (nmn::tt_dec_config((uint64_t)dim, shape, n_cores, max_rank, 1e-4f, &c, nullptr, 0) != NMN_OK) return 0;
    return c.on_device() ? c.lds_floats : ~0ull;
}

extern "C" nmn_status nmn_tt_decompose(const float* vectors, uint64_t n, uint64_t dim, const uint32_t* shape, uint32_t n_cores,
                                       uint32_t max_rank, float tolerance, uint32_t* status_out, uint32_t* ranks_out,
                                       uint64_t* core_off_out, float* cores_out, uint64_t cores_cap) {
    using namespace nmn;
    TTDecConfig c;
    nmn_status st = tt_dec_config(dim, shape, n_cores, max_rank, tolerance, &c, nullptr, 0);
    if (st != NMN_OK) return st;
    if (n == 0) return NMN_OK;
    if (!vectors || !status_out || !ranks_out || (cores_out && !core_off_out)) return set_error(NMN_ERR_INVALID_ARGUMENT, "null argument");
    if (n > (1ull << 31)) return set_error(NMN_ERR_INVALID_ARGUMENT, "TT: more than 2^31 vectors");
    const size_t rk = (size_t)n * (n_cores + 1);
    std::vector<float> slots(cores_out ? (size_t)n * c.slot : 0);
    std::vector<uint32_t> status(n), ranks(rk);
    if (tt_decompose_on_host(c, n)) {
        tt_decompose_host_batch(c, vectors, n, status.data(), ranks.data(), cores_out ? slots.data() : nullptr,
                                env_u32("NMN_TT_DECOMPOSE_HOST_THREADS", 16));
    } else {
        float *d_vec = nullptr, *d_cores = nullptr;
        uint32_t *d_status = nullptr, *d_ranks = nullptr;
        auto body = [&]() -> nmn_status {
            TT_TRY(hipMalloc((void**)&d_vec, (size_t)n * dim * 4));
            TT_TRY(hipMalloc((void**)&d_status, (size_t)n * 4));
            TT_TRY(hipMalloc((void**)&d_ranks, rk * 4));
            if (cores_out) TT_TRY(hipMalloc((void**)&d_cores, std::max<size_t>(slots.size() * 4, 256)));
            TT_TRY(hipMemcpy(d_vec, vectors, (size_t)n * dim * 4, hipMemcpyHostToDevice));
            nmn_status l = launch_tt_decompose(c, d_vec, n, d_status, d_ranks, d_cores, nullptr, nullptr);
            if (l != NMN_OK) return l;
            TT_TRY(hipDeviceSynchronize());
            TT_TRY(hipMemcpy(status.data(), d_status, (size_t)n * 4, hipMemcpyDeviceToHost));
            TT_TRY(hipMemcpy(ranks.data(), d_ranks, rk * 4, hipMemcpyDeviceToHost));
            if (cores_out && !slots.empty()) TT_TRY(hipMemcpy(slots.data(), d_cores, slots.size() * 4, hipMemcpyDeviceToHost));
            return NMN_OK;
        };
        st = body();
        for (void* p : {(void*)d_vec, (void*)d_cores, (void*)d_status, (void*)d_ranks})
            if (p) (void)hipFree(p);
        if (st != NMN_OK) return st;
    }
    // the trains leave their slots for a packed array: core_off as nmn_tt_reconstruct, nmn_tt_norm and nmn_hnsw_search_tt take it
    uint64_t total = 0;
    std::vector<uint64_t> sizes(n, 0);
    for (uint64_t q = 0; q < n; q++) {
        if (status[q] != kTTStatusOk) continue;
        const uint32_t* r = ranks.data() + q * (n_cores + 1);
        for (uint32_t k = 0; k < n_cores; k++) sizes[q] += (uint64_t)r[k] * shape[k] * r[k + 1];
        total += sizes[q];
    }
    if (cores_out && total > cores_cap) {
        char text[160];
        snprintf(text, sizeof text, "TT: cores_cap is %llu floats, the trains need %llu (n * nmn_tt_max_storage always suffices)",
                 (unsigned long long)cores_cap, (unsigned long long)total);
        return set_error(NMN_ERR_INVALID_ARGUMENT, text);
    }
    memcpy(status_out, status.data(), (size_t)n * 4);
    memcpy(ranks_out, ranks.data(), rk * 4);
    if (core_off_out) {
        core_off_out[0] = 0;
        for (uint64_t q = 0; q < n; q++) {
            if (cores_out && sizes[q]) memcpy(cores_out + core_off_out[q], slots.data() + q * c.slot, sizes[q] * 4);
            core_off_out[q + 1] = core_off_out[q] + sizes[q];
        }
    }
    return NMN_OK;
}

extern "C" nmn_status nmn_tt_decompose_device(const float* vectors_dev, uint64_t n, uint64_t dim, const uint32_t* shape,
                                              uint32_t n_cores, uint32_t max_rank, float tolerance, uint32_t* status_dev,
                                              uint32_t* ranks_dev, uint64_t* core_off_dev, float* cores_dev, uint64_t cores_cap,
                                              void* stream) {
    using namespace nmn;
    TTDecConfig c;
    nmn_status st = tt_dec_config(dim, shape, n_cores, max_rank, tolerance, &c, nullptr, 0);
    if (st != NMN_OK) return st;
    if (n == 0) return NMN_OK;
    if (!vectors_dev || !status_dev || !ranks_dev) return set_error(NMN_ERR_INVALID_ARGUMENT, "null argument");
    if (n > (1ull << 31)) return set_error(NMN_ERR_INVALID_ARGUMENT, "TT: more than 2^31 vectors");
    if (cores_dev && cores_cap / c.slot < n) return set_error(NMN_ERR_INVALID_ARGUMENT, "TT: cores_cap is below n * nmn_tt_max_storage");
    return launch_tt_decompose(c, vectors_dev, n, status_dev, ranks_dev, cores_dev, cores_dev ? core_off_dev : nullptr,
                               (hipStream_t)stream);
}

extern "C" nmn_status nmn_tt_reconstruct(const uint32_t* shape, uint32_t n_cores, const uint32_t* ranks, const uint64_t* core_off,
                                         const float* cores, uint32_t nq, float* out_rows) {
    if (nq && !out_rows) return nmn::set_error(NMN_ERR_INVALID_ARGUMENT, "null argument");
    return nmn::tt_public(shape, n_cores, ranks, core_off, cores, nq, out_rows, nullptr);
}

extern "C" nmn_status nmn_tt_norm(const uint32_t* shape, uint32_t n_cores, const uint32_t* ranks, const uint64_t* core_off,
                                  const float* cores, uint32_t nq, float* out_norms) {
    if (nq && !out_norms) return nmn::set_error(NMN_ERR_INVALID_ARGUMENT, "null argument");
    return nmn::tt_public(shape, n_cores, ranks, core_off, cores, nq, nullptr, out_norms);
}

namespace nmn {
namespace {

// One set of a host-buffer similarity call, checked: which trains the kernels take and which the host restatement (`big`: a rank
// above kTTMaxRank or more than kTTMaxStorage core floats; every train when the call goes to the host)
struct TTHostSet {
    const uint32_t* shape = nullptr;
    uint32_t n_cores = 0, n = 0;
    const uint32_t* ranks = nullptr;
    const uint64_t* core_off = nullptr;
    const float* cores = nullptr;
    std::vector<uint8_t> big;
    uint32_t n_big = 0, max_rank = 1;
    uint64_t max_storage = 1;  // over the trains the kernels take
    const uint32_t* ranks_of(uint32_t i) const { return ranks + (size_t)i * (n_cores + 1); }
    const float* cores_of(uint32_t i) const { return cores + core_off[i]; }
    float self_dot(uint32_t i) const { return tt_dot_host(shape, n_cores, ranks_of(i), cores_of(i), ranks_of(i), cores_of(i)); }
};

nmn_status sim_check_set(const char* name, const uint32_t* shape, uint32_t n_cores, const uint32_t* ranks, const uint64_t* core_off,
                         const float* cores, uint32_t n, TTHostSet* s) {
    char buf[320];
    if (!core_off) {
        snprintf(buf, sizeof buf, "TT similarity: %s set: null argument", name);
        return set_error(NMN_ERR_INVALID_ARGUMENT, buf);
    }
    TTBatch b;
    const nmn_status st = tt_check(shape, n_cores, ranks, true, core_off, n, false, &b);
    if (st != NMN_OK) {  // tt_check's text names the train and the rule; the set is named here
        const char* e = nmn_last_error();
        const bool one = !strncmp(e, "TT: query ", 10);
        snprintf(buf, sizeof buf, one ? "TT similarity: %s set: train %s" : "TT similarity: %s set: %s", name, one ? e + 10 : e);
        return set_error(st, buf);
    }
    if (core_off[n] > core_off[0] && !cores) {
        snprintf(buf, sizeof buf, "TT similarity: %s set: null argument", name);
        return set_error(NMN_ERR_INVALID_ARGUMENT, buf);
    }
    s->shape = shape;
    s->n_cores = n_cores;
    s->n = n;
    s->ranks = ranks;
    s->core_off = core_off;
    s->cores = cores;
    s->big.assign(n, 0);
    for (uint32_t i = 0; i < n; i++) {
        const uint32_t* r = s->ranks_of(i);
        uint32_t top = 1;
        for (uint32_t k = 0; k <= n_cores; k++) top = std::max(top, r[k]);
        const uint64_t storage = core_off[i + 1] - core_off[i];
        if (top > kTTMaxRank || storage > kTTMaxStorage) {
            s->big[i] = 1;
            s->n_big++;
        } else {
            s->max_rank = std::max(s->max_rank, top);
            s->max_storage = std::max(s->max_storage, storage);
        }
    }
    return NMN_OK;
}

void all_to_host(TTHostSet* s) {
    s->big.assign(s->n, 1);
    s->n_big = s->n;
}

// fn(lo, hi) over [0, n) on up to NMN_TT_SIMILARITY_HOST_THREADS threads (16), four items a thread at the least
template <class F>
void sim_host_for(uint64_t n, F fn) {
    const uint64_t threads = std::min<uint64_t>(std::max(env_u32("NMN_TT_SIMILARITY_HOST_THREADS", 16), 1u), std::max<uint64_t>(n / 4, 1));
    if (threads <= 1) return fn((uint64_t)0, n);
    std::vector<std::thread> pool;
    for (uint64_t t = 0; t < threads; t++) pool.emplace_back(fn, n * t / threads, n * (t + 1) / threads);
    for (std::thread& t : pool) t.join();
}

// The device copy of one host set: the cores from core_off[0] on, the offsets rebased, skip = big
struct TTDevSet {
    float *cores = nullptr, *self = nullptr;
    uint32_t* ranks = nullptr;
    uint64_t* off = nullptr;
    uint8_t* skip = nullptr;
    TTSimSet set;
    ~TTDevSet() {
        for (void* p : {(void*)cores, (void*)self, (void*)ranks, (void*)off, (void*)skip})
            if (p) (void)hipFree(p);
    }
    nmn_status upload(const TTHostSet& h, bool want_self) {
        const uint64_t c0 = h.core_off[0], cn = h.core_off[h.n] - c0;
        const size_t rk = (size_t)h.n * (h.n_cores + 1);
        std::vector<uint64_t> o(h.core_off, h.core_off + h.n + 1);
        for (uint64_t& x : o) x -= c0;
        TT_TRY(hipMalloc((void**)&cores, std::max<size_t>(cn * 4, 256)));
        TT_TRY(hipMalloc((void**)&ranks, rk * 4));
        TT_TRY(hipMalloc((void**)&off, (size_t)(h.n + 1) * 8));
        TT_TRY(hipMalloc((void**)&skip, h.n));
        if (want_self) TT_TRY(hipMalloc((void**)&self, (size_t)h.n * 4));
        if (cn) TT_TRY(hipMemcpy(cores, h.cores + c0, cn * 4, hipMemcpyHostToDevice));
        TT_TRY(hipMemcpy(ranks, h.ranks, rk * 4, hipMemcpyHostToDevice));
        TT_TRY(hipMemcpy(off, o.data(), (size_t)(h.n + 1) * 8, hipMemcpyHostToDevice));
        TT_TRY(hipMemcpy(skip, h.big.data(), h.n, hipMemcpyHostToDevice));
        set.ranks_dev = ranks;
        set.core_off_dev = off;
        set.cores_dev = cores;
        set.skip_dev = h.n_big ? skip : nullptr;
        set.stride = h.max_storage;
        set.cap = cn;
        set.n = h.n;
        set.max_rank = h.max_rank;
        return NMN_OK;
    }
};

bool sim_on_host(uint64_t work) { return host_forced() || work < env_u32("NMN_TT_SIMILARITY_MIN", kTTSimMinDefault); }

// self[i] = tt_dot_product(t_i, t_i) for every train of the set: the kernel's trains from d (already launched into d.self on the
// null stream and waited for), the others by the host restatement
nmn_status sim_collect_self(const TTHostSet& h, const TTDevSet* d, std::vector<float>* self) {
    self->assign(h.n, 0.0f);
    if (d && h.n_big < h.n) TT_TRY(hipMemcpy(self->data(), d->self, (size_t)h.n * 4, hipMemcpyDeviceToHost));
    std::vector<uint32_t> todo;
    for (uint32_t i = 0; i < h.n; i++)
        if (h.big[i]) todo.push_back(i);
    sim_host_for(todo.size(), [&](uint64_t lo, uint64_t hi) {
        for (uint64_t j = lo; j < hi; j++) (*self)[todo[j]] = h.self_dot(todo[j]);
    });
    return NMN_OK;
}

nmn_status sim_run(uint32_t op, TTHostSet& Q, TTHostSet& T, float* out) {
    const uint64_t pairs = (uint64_t)Q.n * T.n;
    const bool need_self = op != NMN_TT_SIM_DOT;
    if (sim_on_host(pairs)) {
        all_to_host(&Q);
        all_to_host(&T);
    }
    const bool device = Q.n_big < Q.n && T.n_big < T.n;
    if (!device) {  // one set has no train for the kernel: there is no pair for it, so the self dots are the host's as well
        all_to_host(&Q);
        all_to_host(&T);
    }
    std::vector<float> res(pairs), self_q, self_t;
    TTDevSet dq, dt;
    if (device) {
        nmn_status st = dq.upload(Q, need_self);
        if (st == NMN_OK) st = dt.upload(T, need_self);
        if (st != NMN_OK) return st;
        float* d_out = nullptr;
        auto body = [&]() -> nmn_status {
            TT_TRY(hipMalloc((void**)&d_out, pairs * 4));
            if (need_self) {
                TT_TRY(launch_tt_self_dot(Q.shape, Q.n_cores, dq.set, dq.self, nullptr));
                TT_TRY(launch_tt_self_dot(Q.shape, Q.n_cores, dt.set, dt.self, nullptr));
            }
            TT_TRY(launch_tt_similarity(op, Q.shape, Q.n_cores, dq.set, dt.set, dq.self, dt.self, d_out, nullptr));
            TT_TRY(hipDeviceSynchronize());
            TT_TRY(hipMemcpy(res.data(), d_out, pairs * 4, hipMemcpyDeviceToHost));
            return NMN_OK;
        };
        const nmn_status st2 = body();
        if (d_out) (void)hipFree(d_out);
        if (st2 != NMN_OK) return st2;
    }
    if (Q.n_big || T.n_big) {  // the pairs a train above the limits takes part in: the host restatement, same bits
        if (need_self) {
            nmn_status st = sim_collect_self(Q, device ? &dq : nullptr, &self_q);
            if (st == NMN_OK) st = sim_collect_self(T, device ? &dt : nullptr, &self_t);
            if (st != NMN_OK) return st;
        }
        std::vector<uint64_t> todo;
        for (uint32_t i = 0; i < Q.n; i++)
            for (uint32_t j = 0; j < T.n; j++)
                if (Q.big[i] || T.big[j]) todo.push_back((uint64_t)i * T.n + j);
        sim_host_for(todo.size(), [&](uint64_t lo, uint64_t hi) {
            for (uint64_t p = lo; p < hi; p++) {
                const uint32_t i = (uint32_t)(todo[p] / T.n), j = (uint32_t)(todo[p] % T.n);
                const float dot = tt_dot_host(Q.shape, Q.n_cores, Q.ranks_of(i), Q.cores_of(i), T.ranks_of(j), T.cores_of(j));
                res[todo[p]] = tt_sim_finish(op, dot, need_self ? self_q[i] : 0.0f, need_self ? self_t[j] : 0.0f);
            }
        });
    }
    memcpy(out, res.data(), pairs * 4);
    return NMN_OK;
}

nmn_status self_dot_run(TTHostSet& S, float* out) {
    if (sim_on_host(S.n)) all_to_host(&S);
    std::vector<float> self;
    TTDevSet d;
    const bool device = S.n_big < S.n;
    if (device) {
        const nmn_status st = d.upload(S, true);
        if (st != NMN_OK) return st;
        TT_TRY(launch_tt_self_dot(S.shape, S.n_cores, d.set, d.self, nullptr));
        TT_TRY(hipDeviceSynchronize());
    }
    const nmn_status st = sim_collect_self(S, device ? &d : nullptr, &self);
    if (st != NMN_OK) return st;
    memcpy(out, self.data(), (size_t)S.n * 4);
    return NMN_OK;
}

// what the device entries can check of one set on the host
nmn_status sim_device_set(const char* name, const uint32_t* ranks_dev, const uint64_t* core_off_dev, const float* cores_dev,
                          uint64_t stride, const uint32_t* status_dev, uint32_t n, TTSimSet* s) {
    char buf[160];
    if (!ranks_dev || !cores_dev) {
        snprintf(buf, sizeof buf, "TT similarity: %s set: null argument", name);
        return set_error(NMN_ERR_INVALID_ARGUMENT, buf);
    }
    if (stride < 1 || stride > kTTMaxStorage) {
        snprintf(buf, sizeof buf, "TT similarity: %s set: stride must be 1..%u floats (nmn_tt_limits)", name, kTTMaxStorage);
        return set_error(NMN_ERR_INVALID_ARGUMENT, buf);
    }
    s->ranks_dev = ranks_dev;
    s->core_off_dev = core_off_dev;
    s->cores_dev = cores_dev;
    s->status_dev = status_dev;
    s->stride = stride;
    s->cap = (uint64_t)n * stride;
    s->n = n;
    s->max_rank = kTTMaxRank;
    return NMN_OK;
}

nmn_status sim_device_shape(const uint32_t* shape, uint32_t n_cores) {
    if (n_cores < 1 || n_cores > kTTMaxCores) return set_error(NMN_ERR_INVALID_ARGUMENT, "TT: n_cores must be 1..8");
    if (!shape) return set_error(NMN_ERR_INVALID_ARGUMENT, "null argument");
    for (uint32_t k = 0; k < n_cores; k++)
        if (shape[k] < 1) return set_error(NMN_ERR_INVALID_ARGUMENT, "TT: every mode of the shape must be >= 1");
    return NMN_OK;
}

constexpr uint32_t kTTSimMaxTrains = 1u << 31;

}  // namespace
}  // namespace nmn

extern "C" nmn_status nmn_tt_similarity(uint32_t op, const uint32_t* shape_q, uint32_t n_cores_q, const uint32_t* ranks_q,
                                        const uint64_t* core_off_q, const float* cores_q, uint32_t nq, const uint32_t* shape_t,
                                        uint32_t n_cores_t, const uint32_t* ranks_t, const uint64_t* core_off_t, const float* cores_t,
                                        uint32_t nt, float* out) {
    using namespace nmn;
    if (op > NMN_TT_SIM_EUCLIDEAN) return set_error(NMN_ERR_INVALID_ARGUMENT, "TT similarity: unknown op");
    if (nq == 0 || nt == 0) return NMN_OK;
    if (!out) return set_error(NMN_ERR_INVALID_ARGUMENT, "null argument");
    if (nq > kTTSimMaxTrains || nt > kTTSimMaxTrains) return set_error(NMN_ERR_INVALID_ARGUMENT, "TT similarity: more than 2^31 trains in a set");
    TTHostSet Q, T;
    nmn_status st = sim_check_set("query", shape_q, n_cores_q, ranks_q, core_off_q, cores_q, nq, &Q);
    if (st == NMN_OK) st = sim_check_set("target", shape_t, n_cores_t, ranks_t, core_off_t, cores_t, nt, &T);
    if (st != NMN_OK) return st;
    if (n_cores_q != n_cores_t || memcmp(shape_q, shape_t, n_cores_q * sizeof(uint32_t)))
        return set_error(NMN_ERR_INVALID_ARGUMENT, "incompatible TT shapes for operation");
    return sim_run(op, Q, T, out);
}

extern "C" nmn_status nmn_tt_self_dot(const uint32_t* shape, uint32_t n_cores, const uint32_t* ranks, const uint64_t* core_off,
                                      const float* cores, uint32_t n, float* out) {
    using namespace nmn;
    if (n == 0) return NMN_OK;
    if (!out) return set_error(NMN_ERR_INVALID_ARGUMENT, "null argument");
    if (n > kTTSimMaxTrains) return set_error(NMN_ERR_INVALID_ARGUMENT, "TT similarity: more than 2^31 trains in a set");
    TTHostSet S;
    const nmn_status st = sim_check_set("train", shape, n_cores, ranks, core_off, cores, n, &S);
    if (st != NMN_OK) return st;
    return self_dot_run(S, out);
}

extern "C" nmn_status nmn_tt_self_dot_device(const uint32_t* shape, uint32_t n_cores, const uint32_t* ranks_dev,
                                             const uint64_t* core_off_dev, const float* cores_dev, uint64_t stride,
                                             const uint32_t* status_dev, uint32_t n, float* out_dev, void* stream) {
    using namespace nmn;
    nmn_status st = sim_device_shape(shape, n_cores);
    if (st != NMN_OK) return st;
    if (n == 0) return NMN_OK;
    if (!out_dev) return set_error(NMN_ERR_INVALID_ARGUMENT, "null argument");
    if (n > kTTSimMaxTrains) return set_error(NMN_ERR_INVALID_ARGUMENT, "TT similarity: more than 2^31 trains in a set");
    TTSimSet s;
    st = sim_device_set("train", ranks_dev, core_off_dev, cores_dev, stride, status_dev, n, &s);
    if (st != NMN_OK) return st;
    TT_TRY(launch_tt_self_dot(shape, n_cores, s, out_dev, (hipStream_t)stream));
    return NMN_OK;
}

extern "C" nmn_status nmn_tt_similarity_device(uint32_t op, const uint32_t* shape, uint32_t n_cores, const uint32_t* ranks_q_dev,
                                               const uint64_t* core_off_q_dev, const float* cores_q_dev, uint64_t stride_q,
                                               const uint32_t* status_q_dev, uint32_t nq, const uint32_t* ranks_t_dev,
                                               const uint64_t* core_off_t_dev, const float* cores_t_dev, uint64_t stride_t,
                                               const uint32_t* status_t_dev, uint32_t nt, const float* self_q_dev,
                                               const float* self_t_dev, float* out_dev, void* stream) {
    using namespace nmn;
    if (op > NMN_TT_SIM_EUCLIDEAN) return set_error(NMN_ERR_INVALID_ARGUMENT, "TT similarity: unknown op");
    nmn_status st = sim_device_shape(shape, n_cores);
    if (st != NMN_OK) return st;
    if (nq == 0 || nt == 0) return NMN_OK;
    if (!out_dev || (op != NMN_TT_SIM_DOT && (!self_q_dev || !self_t_dev))) return set_error(NMN_ERR_INVALID_ARGUMENT, "null argument");
    if (nq > kTTSimMaxTrains || nt > kTTSimMaxTrains) return set_error(NMN_ERR_INVALID_ARGUMENT, "TT similarity: more than 2^31 trains in a set");
    TTSimSet q, t;
    st = sim_device_set("query", ranks_q_dev, core_off_q_dev, cores_q_dev, stride_q, status_q_dev, nq, &q);
    if (st == NMN_OK) st = sim_device_set("target", ranks_t_dev, core_off_t_dev, cores_t_dev, stride_t, status_t_dev, nt, &t);
    if (st != NMN_OK) return st;
    TT_TRY(launch_tt_similarity(op, shape, n_cores, q, t, self_q_dev, self_t_dev, out_dev, (hipStream_t)stream));
    return NMN_OK;
}

extern "C" nmn_status nmn_tt_limits(uint32_t* max_cores, uint32_t* max_rank, uint32_t* max_storage, uint32_t* max_level) {
    if (max_cores) *max_cores = nmn::kTTMaxCores;
    if (max_rank) *max_rank = nmn::kTTMaxRank;
    if (max_storage) *max_storage = nmn::kTTMaxStorage;
    if (max_level) *max_level = nmn::kTTMaxLevel;
    return NMN_OK;
}
