// nmn_tt.h — tensor-train queries (tensor_compress/src/tensor_train.rs): what nmn_tt.hip offers the HNSW walk (nmn_hnsw.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

#include "neumann_gpu.h"

namespace nmn {

// The limits of the device path (docs/hnsw.md §17).  One workgroup prepares one train with everything in LDS: its cores
// (kTTMaxStorage floats), two reconstruction levels (kTTMaxLevel floats each: level k holds n_1 .. n_k vectors of length r_k; the
// last level goes straight to HBM) and two Gram matrices (kTTMaxRank^2 floats each) — just under the 64 KiB a workgroup may use.
constexpr uint32_t kTTMaxCores = 8;
constexpr uint32_t kTTMaxRank = 32;
constexpr uint32_t kTTMaxStorage = 8192;
constexpr uint32_t kTTMaxLevel = 3056;
constexpr uint32_t kTTGridMax = 256;  // workgroups of one launch; the queries beyond are taken in a grid-stride loop

// One call's trains as the entries take them, checked.  ranks: [nq][n_cores + 1], or one vector for all (per_query == false).
struct TTBatch {
    uint32_t n_cores = 0, nq = 0;
    uint64_t dim = 0;
    uint32_t shape[kTTMaxCores] = {};
    const uint32_t* ranks = nullptr;
    bool per_query = true;
    const uint64_t* core_off = nullptr;  // [nq + 1] into cores, or null: query q starts at q * storage(0)
    const float* cores = nullptr;
    std::vector<uint8_t> on_host;        // [nq] 1: the train is above the LDS limits, the host restatement prepares it
    uint32_t n_on_host = 0;
    const uint32_t* ranks_of(uint32_t q) const { return ranks + (per_query ? (size_t)q * (n_cores + 1) : 0); }
    uint64_t storage_of(uint32_t q) const {
        const uint32_t* r = ranks_of(q);
        uint64_t s = 0;
        for (uint32_t k = 0; k < n_cores; k++) s += (uint64_t)r[k] * shape[k] * r[k + 1];
        return s;
    }
    uint64_t offset_of(uint32_t q) const { return core_off ? core_off[q] : (uint64_t)q * storage_of(0); }
};

// Every rule of a well-formed train (neumann_gpu.h, nmn_tt_reconstruct), for every query, before anything is enqueued or written;
// the text names the query and the rule.  core_off null: one rank vector, the trains back to back.  Fills b, on_host included;
// host_env: NMN_HNSW_HOST_SEARCH=1 sends every train to the host restatement.
nmn_status tt_check(const uint32_t* shape, uint32_t n_cores, const uint32_t* ranks, bool per_query, const uint64_t* core_off,
                    uint32_t nq, bool host_env, TTBatch* b);

// tt_reconstruct (tensor_train.rs:401-436) and tt_norm (440-474) of one train on the host, the reference's loops restated
void tt_reconstruct_host(const uint32_t* shape, uint32_t n_cores, const uint32_t* ranks, const float* cores, float* out);
float tt_norm_host(const uint32_t* shape, uint32_t n_cores, const uint32_t* ranks, const float* cores);
// the magnitude the walk divides by: a norm below 1e-10 is 0.0 (cosine_distance_tt_with_norm, hnsw.rs:1199-1201)
inline float tt_walk_magnitude(float norm) { return norm < 1e-10f ? 0.0f : norm; }

// One launch over b.nq trains whose cores are in DEVICE memory (cores_dev laid out as b.cores is; ranks_dev / core_off_dev the
// device copies of b.ranks / b.core_off when per_query / core_off are set, null otherwise; skip_dev [nq] nullable: 1 = leave the
// query to the host).  Each output is nullable: rows [nq][dim], the raw norms [nq], the walk's magnitudes [nq].
hipError_t launch_tt_prepare(const TTBatch& b, const float* cores_dev, const uint32_t* ranks_dev, const uint64_t* core_off_dev,
                             const uint8_t* skip_dev, float* rows_dev, float* norms_dev, float* mags_dev, hipStream_t s);

// ---- tt_decompose (tensor_train.rs:315-397), docs/hnsw.md §21 ----------------------------------------------------------------

// The device path of tt_decompose keeps one vector's whole state in the dynamic LDS of its workgroup; a config is served there when
// tt_decompose_lds_floats(config) <= kTTDecMaxLdsFloats (64 KiB, the most a workgroup may ask for without an attribute, two such
// workgroups on the 160 KiB of a CU) and no worst-case rank is above kTTDecMaxRank.
constexpr uint32_t kTTDecMaxLdsFloats = 16384;
constexpr uint32_t kTTDecMaxRank = 64;
constexpr uint32_t kTTDecGridMax = 4096;     // workgroups of one launch (NMN_TT_DECOMPOSE_GRID), the vectors beyond in a stride loop
constexpr uint32_t kTTDecThreads = 64;       // one wave owns a vector (NMN_TT_DECOMPOSE_THREADS: 64, 128 or 256), docs/hnsw.md §21
constexpr uint32_t kTTDecMinDefault = 320;   // NMN_TT_DECOMPOSE_MIN: calls of fewer vectors are decomposed by the host (measured, §21)
constexpr uint32_t kTTStatusOk = 0, kTTStatusEmptyMatrix = 1;

// One call's config, checked (tt_decompose's own three checks are the entries'): the worst-case ranks
// rb[k + 1] = min(max_rank, rb[k] * shape[k], shape[k + 1] * .. * shape[n_cores - 1]) and the slot of one train.
struct TTDecConfig {
    uint32_t n_cores = 0, max_rank = 0;
    float tolerance = 0.0f;
    uint64_t dim = 0;
    uint32_t shape[kTTMaxCores] = {};
    uint32_t rb[kTTMaxCores + 1] = {};
    uint64_t slot = 0;        // sum of rb[k] * shape[k] * rb[k + 1]: nmn_tt_max_storage
    uint64_t lds_floats = 0;  // what tt_decompose_kernel needs for this config
    bool on_device() const;   // within the limits above
};
// NMN_ERR_INVALID_ARGUMENT with the reference's Display text for tt_decompose's three argument errors (dim == 0: "empty vector"; the
// product of the shape != dim: "dimension .. cannot be reshaped to .."; max_rank < 1: "invalid TT-rank: must be >= 1"), and for an
// n_cores outside 1..8.  `debug` (nullable) receives the Debug form of the TTError.
nmn_status tt_dec_config(uint64_t dim, const uint32_t* shape, uint32_t n_cores, uint32_t max_rank, float tolerance, TTDecConfig* c,
                         char* debug, size_t debug_cap);

// tt_decompose of one vector on the host, the reference's loops restated: ranks_out [n_cores + 1] (zeros when the status is
// EmptyMatrix), cores_out nullable (status only), the cores back to back.  Returns kTTStatusOk or kTTStatusEmptyMatrix.
uint32_t tt_decompose_host(const TTDecConfig& c, const float* vector, uint32_t* ranks_out, float* cores_out);
// n vectors: the host restatement on up to `threads` threads (the vectors are independent); slots at q * c.slot
void tt_decompose_host_batch(const TTDecConfig& c, const float* vectors, uint64_t n, uint32_t* status, uint32_t* ranks, float* cores,
                             unsigned threads);
// true: this call of n vectors goes to the host (NMN_HNSW_HOST_SEARCH=1, a config above the limits, n < NMN_TT_DECOMPOSE_MIN)
bool tt_decompose_on_host(const TTDecConfig& c, uint64_t n);
// One launch on `s` over n vectors in DEVICE memory: status_dev [n], ranks_dev [n][n_cores + 1], cores_dev nullable (status only),
// train q at q * c.slot.  The config must be on_device().  The Gaussian matrices of the randomized path are made on the host once
// per config and device and kept.  core_off_dev nullable: [n + 1], q * c.slot.
nmn_status launch_tt_decompose(const TTDecConfig& c, const float* vectors_dev, uint64_t n, uint32_t* status_dev, uint32_t* ranks_dev,
                               float* cores_dev, uint64_t* core_off_dev, hipStream_t s);

// ---- tt_dot_product, tt_cosine_similarity, tt_euclidean_distance (tensor_train.rs:480-546), docs/hnsw.md §23 -------------------

// The device path compares trains within kTTMaxCores, kTTMaxRank and kTTMaxStorage (kTTMaxLevel does not apply: nothing is
// reconstructed).  A workgroup keeps one query's cores and, per wave, two Gram matrices in dynamic LDS, under the 64 KiB a
// workgroup may ask for without an attribute.
constexpr uint32_t kTTSimMaxLdsFloats = 16368;  // (16 floats short of 64 KiB: the kernel's static LDS)
constexpr uint32_t kTTSimGridMax = 2048;        // workgroups of one launch (NMN_TT_SIMILARITY_GRID), the work beyond in a stride loop
constexpr uint32_t kTTSimMinDefault = 32;       // NMN_TT_SIMILARITY_MIN: calls of fewer pairs are the host's (measured, docs/hnsw.md §23)

// One core step of tt_dot_product (tensor_train.rs:480-516) for one pair by one wave: the lanes share out the r2a * r2b outputs,
// each output one sequential chain from +0.0 over k, then ia, then ib of (gram[ia * r1b + ib] * A[ia, k, x]) * B[ib, k, y].  A, B:
// the pair's k-th cores, in global memory or LDS; gram: r1a * r1b floats in LDS; nxt: r2a * r2b floats in LDS.  Shared by
// tt_similarity_kernel / tt_self_dot_kernel (nmn_tt.hip) and the TTN walk (nmn_hnsw_kernels.hip): both translation units are built
// with -ffp-contract=off, so no product is fused into its addition in either.
__device__ __forceinline__ void tt_gram_step(const float* __restrict__ A, const float* __restrict__ B, const float* gram, float* nxt,
                                             uint32_t r1a, uint32_t r2a, uint32_t r1b, uint32_t r2b, uint32_t n, uint32_t lane) {
    for (uint32_t o = lane; o < r2a * r2b; o += 64) {
        const uint32_t x = o / r2b, y = o - x * r2b;
        float sum = 0.0f;
        for (uint32_t kk = 0; kk < n; kk++)
            for (uint32_t ia = 0; ia < r1a; ia++) {
                const float ga = A[(ia * n + kk) * r2a + x];
                for (uint32_t ib = 0; ib < r1b; ib++) {
                    const float t = gram[ia * r1b + ib] * ga;
                    const float p = t * B[(ib * n + kk) * r2b + y];
                    sum = sum + p;
                }
            }
        nxt[o] = sum;
    }
}

// tt_dot_product of two trains of one shape on the host, the reference's loops restated; with a == b the chain of tt_norm
float tt_dot_host(const uint32_t* shape, uint32_t n_cores, const uint32_t* ranks_a, const float* cores_a, const uint32_t* ranks_b,
                  const float* cores_b);

// One set of n trains in DEVICE memory: per-train ranks [n][n_cores + 1]; train i's cores at core_off_dev[i] (core_off_dev [n + 1]),
// or at i * stride when core_off_dev is null; no train holds more than `stride` floats and the buffer holds `cap`.  status_dev
// (nullable): NMN_TT_OK per good train.  skip_dev (nullable): 1 = nothing this train takes part in is computed or written.
// max_rank: the largest rank of any train that is not skipped, kTTMaxRank when the host cannot know.  The kernels check every
// train against all of this before they read through its ranks; a train that fails leaves the quiet NaN 0x7FC00000.
struct TTSimSet {
    const uint32_t* ranks_dev = nullptr;
    const uint64_t* core_off_dev = nullptr;
    const float* cores_dev = nullptr;
    const uint32_t* status_dev = nullptr;
    const uint8_t* skip_dev = nullptr;
    uint64_t stride = 0, cap = 0;
    uint32_t n = 0, max_rank = kTTMaxRank;
};
// out_dev[i] = tt_dot_product(t_i, t_i), one launch on `s`
hipError_t launch_tt_self_dot(const uint32_t* shape, uint32_t n_cores, const TTSimSet& set, float* out_dev, hipStream_t s);
// out_dev[q.n][t.n] = op (NMN_TT_SIM_*) of (query i, target j), one launch on `s`; self_*_dev: what launch_tt_self_dot wrote, read
// for cosine and Euclidean only
hipError_t launch_tt_similarity(uint32_t op, const uint32_t* shape, uint32_t n_cores, const TTSimSet& q, const TTSimSet& t,
                                const float* self_q_dev, const float* self_t_dev, float* out_dev, hipStream_t s);

}  // namespace nmn
