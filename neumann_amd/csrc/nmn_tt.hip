// nmn_tt.hip — tensor-train vectors prepared on the GPU: tt_reconstruct (tensor_compress/src/tensor_train.rs:401-436) and tt_norm
// (440-474), bit for bit, for the TT queries of the HNSW walk (HNSWIndex::search_tt_with_ef, tensor_store/src/hnsw.rs:1811-1841)
// and for insert_tt_vector (1755-1759).  docs/hnsw.md §17.
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
}  // namespace nmn

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

extern "C" nmn_status nmn_tt_limits(uint32_t* max_cores, uint32_t* max_rank, uint32_t* max_storage, uint32_t* max_level) {
    if (max_cores) *max_cores = nmn::kTTMaxCores;
    if (max_rank) *max_rank = nmn::kTTMaxRank;
    if (max_storage) *max_storage = nmn::kTTMaxStorage;
    if (max_level) *max_level = nmn::kTTMaxLevel;
    return NMN_OK;
}
