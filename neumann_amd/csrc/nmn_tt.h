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

}  // namespace nmn
