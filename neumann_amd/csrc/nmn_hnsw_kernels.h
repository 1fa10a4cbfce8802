// nmn_hnsw_kernels.h — the arguments of the three HNSW kernels and the launchers of nmn_hnsw_kernels.hip, the only translation
// unit of the index with __global__ code (docs/hnsw.md, "Source layout").
#pragma once
#include "nmn_hnsw_arith.h"

namespace nmn {
namespace {

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

// The record of one EmbeddingStorage::TensorTrain node in HBM (docs/hnsw.md §24): where its cores start in the pool, its shape and
// ranks (ranks[0] == ranks[n_cores] == 1), the bits of its cached tt_norm.  96 bytes.
struct TTNodeDev {
    uint32_t off_lo, off_hi, n_cores, norm_bits;
    uint32_t modes[8];
    uint32_t ranks[9];
    uint32_t pad[3];
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
    // hnsw_search_kernel<.., TTN = true> (a TT-query call on a handle with EmbeddingStorage::TensorTrain nodes, docs/hnsw.md §24):
    // the slot of every node (kNone: not a TT node), the record per TT node and the pool of their cores, tt_pool floats long; the
    // call's trains — one shape, ttq_shape[ttq_ncores]; query i's ranks at ttq_ranks + i * (ttq_ncores + 1), or ttq_ranks_u for
    // every query when ttq_ranks is null; its cores at ttq_cores + ttq_off[i], or at i * ttq_stride when ttq_off is null — and the
    // floats of the two LDS regions: ttq_cap for a query's cores, tt_gcap for each of the two Gram buffers.
    const uint32_t* tt_slot;
    const TTNodeDev* tt_rec;
    const float* tt_cores;
    uint64_t tt_pool;
    const float* ttq_cores;
    const uint32_t* ttq_ranks;
    const uint64_t* ttq_off;
    uint64_t ttq_stride;
    uint32_t ttq_ncores, ttq_cap, tt_gcap;
    uint32_t ttq_shape[8], ttq_ranks_u[9];
};

// The LDS a TTN launch adds in front of the heaps, in floats: the query's ranks (16 slots), its cores, two Gram buffers
__host__ __device__ inline uint32_t tt_region_floats(uint32_t qcap, uint32_t gcap) { return 16u + ((qcap + 1u) & ~1u) + 2u * ((gcap + 1u) & ~1u); }

// hnsw_insert_walk_kernel: the build walk of one batch (nmn_hnsw_insert_bulk, docs/hnsw.md §19)
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

}  // namespace

// The launchers, defined in nmn_hnsw_kernels.hip.  The argument structs stay in the unnamed namespace (their names are part of
// the kernels' mangled names), and a type without linkage cannot stand in a signature that crosses translation units: the
// structs cross by address, and the typed wrappers below are what the host code calls.  Geometry: one wave per workgroup.
namespace hnsw {
void launch_search_args(bool spill, bool q8, bool bin, bool perq, int qkind, bool mix, bool ttn, uint32_t grid, size_t lds, hipStream_t s,
                        const void* search_args);
void launch_insert_walk_args(uint32_t grid, size_t lds, hipStream_t s, const void* insert_args);
void launch_patch_args(uint32_t grid, hipStream_t s, const void* patch_args);
}  // namespace hnsw

namespace {
// hnsw_search_kernel<spill, ...>: launch_walk<spill> of nmn_hnsw_kernels.hip picks the instantiation
inline void launch_search(bool spill, bool q8, bool bin, bool perq, int qkind, bool mix, bool ttn, uint32_t grid, size_t lds,
                          hipStream_t s, const SearchArgs& a) {
    hnsw::launch_search_args(spill, q8, bin, perq, qkind, mix, ttn, grid, lds, s, &a);
}
inline void launch_insert_walk(uint32_t grid, size_t lds, hipStream_t s, const InsertArgs& a) {
    hnsw::launch_insert_walk_args(grid, lds, s, &a);
}
inline void launch_patch(uint32_t grid, hipStream_t s, const PatchArgs& a) { hnsw::launch_patch_args(grid, s, &a); }
}  // namespace

}  // namespace nmn
