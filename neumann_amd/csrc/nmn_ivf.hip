// nmn_ivf.hip — IVF-Flat probe on the GPU: `IVFIndex::{add, search_with_nprobe}` of
// tensor_store/src/ivf.rs:276-406 for `IVFStorage::Flat`, on top of the flat-scan kernels.
//
// Layout: the vectors stay in ID (insertion) order in one nmn_index — row == the id `add` returns
// (ivf.rs:288) — plus `assign[row]`, the cluster of each row.  An inverted list is therefore a set of
// rows, not a contiguous range: a probe marks the nprobe nearest clusters, one kernel turns
// `assign` into the selection bitmap (1 bit per row), and the masked scan reads only the selected
// rows (3 KB contiguous each at d = 768).  `add` is an append, never a list reshuffle.
//
// Exactness: every distance the reference computes here is `squared_euclidean` (ivf.rs:500-508), the
// same strictly sequential f32 sum as the flat Euclidean metric, so the exact kernels restate it
// bit for bit: centroids are ranked by the squared distance, ascending, ties by centroid index
// (stable sort of an enumerate, ivf.rs:331-337); list members by `sqrt` of it, ascending; equal
// distances keep candidate order = probe order of the cluster, then list (= id) order (stable sort,
// ivf.rs:402).  `add` picks the first nearest centroid (`min_by`, ivf.rs:490-497).
#include <algorithm>
#include <cmath>
#include <cstring>
#include <mutex>
#include <condition_variable>
#include <memory>
#include <shared_mutex>
#include <new>
#include <vector>

#include "nmn_index.h"

using namespace nmn;

namespace {

constexpr uint32_t kNoRank = 0xFFFFFFFFu;
constexpr uint32_t kAssignChunk = 4096;  // rows assigned per exact sweep over the centroids

// first centroid whose squared distance is minimal, with `min_by`'s fold semantics on NaN
// (core::iter::Iterator::min_by keeps the earlier element unless the later compares strictly Less):
// scores are -d^2 in tile-major layout score_at(c, q, nql); one wave per new row.
__global__ __launch_bounds__(256) void ivf_assign_kernel(const uint32_t* __restrict__ scores, uint32_t n_clusters,
                                                         uint32_t nql, uint32_t nq, uint32_t* __restrict__ assign_out) {
    const uint32_t q = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const uint32_t lane = threadIdx.x & 63u;
    if (q >= nq) return;
    const float first = u2f(scores[score_at(0, q, nql)]);
    float best = -__builtin_inff();
    uint32_t best_c = kNoRank;
    for (uint32_t c = lane; c < n_clusters; c += 64) {
        const float s = u2f(scores[score_at(c, q, nql)]);
        if (s > best || (s == best && c < best_c)) {  // NaN never wins; ties go to the lower index
            best = s;
            best_c = c;
        }
    }
    for (int off = 32; off > 0; off >>= 1) {
        const float ob = __shfl_down(best, off);
        const uint32_t oc = __shfl_down(best_c, off);
        if (ob > best || (ob == best && oc < best_c)) {
            best = ob;
            best_c = oc;
        }
    }
    if (lane == 0) {
        uint32_t c = best_c;
        if (first != first || c == kNoRank) c = 0;  // a NaN first element is never displaced; all-NaN keeps 0
        // -inf everywhere except NaNs: `best_c` may still be kNoRank only when every score is NaN or -inf;
        // with -inf scores the fold keeps the first element as well
        assign_out[q] = c;
    }
}

__global__ void ivf_probe_rank_kernel(const uint64_t* __restrict__ probe_rows, const uint32_t* __restrict__ probe_count,
                                      uint32_t* __restrict__ probe_rank) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < *probe_count) probe_rank[probe_rows[i]] = i;
}

// The whole centroid ranking of one query in one workgroup (n_clusters <= kRankMax): composite keys
// `score key << 32 | ~cluster` (score = -d^2, so descending composite = ascending squared distance, ties by cluster
// index — the reference's stable sort of an enumerate), bitonic sort in LDS, then probe_rows[0..np) = the clusters in
// probe order and probe_rank[cluster] = its rank or kNoRank.  Replaces five launches (keys, 4096-key tile sort, emit,
// memset, rank scatter: ~50 us of a 370 us probe) by one.
constexpr uint32_t kRankMax = 4096;
// Query blockIdx.x of a chunk of nql queries (their scores interleaved tile-major: score_at): outputs at probe_rows + q * n_clusters,
// probe_rank + q * n_clusters, probe_count + q.
__global__ __launch_bounds__(1024) void ivf_rank_kernel(const uint32_t* __restrict__ cscores, uint32_t nql, uint32_t n_clusters,
                                                        uint32_t np2, uint32_t np, uint64_t* __restrict__ probe_rows,
                                                        uint32_t* __restrict__ probe_count,
                                                        uint32_t* __restrict__ probe_rank) {
    __shared__ uint64_t t[kRankMax];
    const uint32_t tid = threadIdx.x, qi = blockIdx.x;
    probe_rows += (size_t)qi * n_clusters;
    probe_rank += (size_t)qi * n_clusters;
    probe_count += qi;
    for (uint32_t i = tid; i < np2; i += 1024) {
        uint64_t key = 0;
        if (i < n_clusters) {
            const uint32_t sk = bits_to_key(cscores[score_at(i, qi, nql)]);
            if (sk != kKeyMasked) key = ((uint64_t)sk << 32) | (uint32_t)~i;
        }
        t[i] = key;
    }
    __syncthreads();
    for (uint32_t size = 2; size <= np2; size <<= 1) {
        for (uint32_t stride = size >> 1; stride > 0; stride >>= 1) {
            for (uint32_t p = tid; p < (np2 >> 1); p += 1024) {
                const uint32_t lo = ((p & ~(stride - 1)) << 1) | (p & (stride - 1));
                const uint32_t hi = lo + stride;
                const bool desc = (lo & size) == 0;
                const uint64_t a = t[lo], b = t[hi];
                if ((a < b) == desc) {
                    t[lo] = b;
                    t[hi] = a;
                }
            }
            __syncthreads();
        }
    }
    for (uint32_t c = tid; c < n_clusters; c += 1024) probe_rank[c] = kNoRank;
    __syncthreads();
    uint32_t mine = 0;
    for (uint32_t i = tid; i < np; i += 1024) {
        const uint64_t key = t[i];
        if (key != 0) {
            const uint32_t c = ~(uint32_t)key;
            probe_rows[i] = c;
            probe_rank[c] = i;
            mine++;
        }
    }
    // participating clusters sort first: count = number of non-zero keys among the first np
    __shared__ uint32_t total;
    if (tid == 0) total = 0;
    __syncthreads();
    if (mine) atomicAdd(&total, mine);
    __syncthreads();
    if (tid == 0) *probe_count = total;
}

// rows [row_lo, n_rows) whose list is probed (the rows below row_lo are served by the list-major copy)
// (query blockIdx.y of a chunk: its ranks at probe_rank + y * n_clusters, its bitmap at mask + y * mask_stride)
__global__ __launch_bounds__(256) void ivf_mask_kernel(const uint32_t* __restrict__ assign,
                                                       const uint32_t* __restrict__ probe_rank, uint32_t n_clusters, uint64_t n_rows,
                                                       uint64_t row_lo, uint64_t* __restrict__ mask, uint64_t mask_stride) {
    probe_rank += (size_t)blockIdx.y * n_clusters;
    mask += (size_t)blockIdx.y * mask_stride;
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t n_words = (n_rows + 63) >> 6;
    const uint64_t wave = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const uint64_t n_waves = ((uint64_t)gridDim.x * blockDim.x) >> 6;
    for (uint64_t w = wave; w < n_words; w += n_waves) {
        uint64_t word = 0ull;
        if (((w + 1) << 6) > row_lo) {  // (wave-uniform: words entirely below row_lo read nothing)
            const uint64_t row = (w << 6) + lane;
            const bool in = row >= row_lo && row < n_rows && probe_rank[assign[row]] != kNoRank;
            word = __ballot(in);
        }
        if (lane == 0) mask[w] = word;
    }
}

// The same selection over the LIST-MAJOR copy: its rows [list_off[c], list_off[c + 1]) are list c, so a probed list is a run of
// set bits and the list scan streams contiguous rows.  No per-row array is read: a lane finds its row's list by bisecting the
// (n_clusters + 1)-entry offset table.
__global__ __launch_bounds__(256) void ivf_range_mask_kernel(const uint32_t* __restrict__ list_off, uint32_t n_clusters,
                                                             const uint32_t* __restrict__ probe_rank, uint64_t n_rows,
                                                             uint64_t* __restrict__ mask, uint64_t mask_stride) {
    probe_rank += (size_t)blockIdx.y * n_clusters;
    mask += (size_t)blockIdx.y * mask_stride;
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t n_words = (n_rows + 63) >> 6;
    const uint64_t wave = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const uint64_t n_waves = ((uint64_t)gridDim.x * blockDim.x) >> 6;
    for (uint64_t w = wave; w < n_words; w += n_waves) {
        const uint64_t row = (w << 6) + lane;
        bool in = false;
        if (row < n_rows) {
            uint32_t lo = 0, hi = n_clusters;  // the list c with list_off[c] <= row < list_off[c + 1]
            while (hi - lo > 1) {
                const uint32_t mid = (lo + hi) >> 1;
                if (list_off[mid] <= (uint32_t)row) lo = mid;
                else hi = mid;
            }
            in = probe_rank[lo] != kNoRank;
        }
        const uint64_t word = __ballot(in);
        if (lane == 0) mask[w] = word;
    }
}

// dst[i][0 .. dim) = src[perm[pos0 + i]][0 .. dim): rows of the id-ordered corpus (stride ld) gathered into a tight block
__global__ __launch_bounds__(256) void ivf_gather_kernel(const float* __restrict__ src, uint32_t ld, uint32_t dim,
                                                         const uint32_t* __restrict__ perm, uint64_t pos0, uint32_t cnt,
                                                         float* __restrict__ dst) {
    for (uint32_t i = blockIdx.x; i < cnt; i += gridDim.x) {
        const float* row = src + (uint64_t)perm[pos0 + i] * ld;
        float* out = dst + (uint64_t)i * dim;
        for (uint32_t c = threadIdx.x; c < dim; c += 256) out[c] = row[c];
    }
}

// A grow-only buffer of search scratch: device memory, or (pinned) host memory the device copies from and to.
struct Grow {
    void* p = nullptr;
    size_t cap = 0;
    bool pinned = false;
    // At least `bytes` (64 at the least); a buffer too small is replaced, its content lost.  `wait`: work enqueued on `s` may still
    // use the old buffer, so `s` is synchronised first — and `wait` cleared, so a run of reservations waits once, and only when
    // something grows.  false: the caller has waited already.
    hipError_t reserve(size_t bytes, hipStream_t s, bool& wait) {
        bytes = std::max<size_t>(bytes, 64);
        if (cap >= bytes) return hipSuccess;
        if (wait) {
            hipError_t e = hipStreamSynchronize(s);
            if (e != hipSuccess) return e;
            wait = false;
        }
        release();
        hipError_t e = pinned ? hipHostMalloc(&p, bytes, hipHostMallocDefault) : hipMalloc(&p, bytes);
        if (e == hipSuccess) cap = bytes;
        return e;
    }
    void release() {
        if (p) (void)(pinned ? hipHostFree(p) : hipFree(p));
        p = nullptr;
        cap = 0;
    }
};
template <class T>
T* gp(const Grow& g) {
    return static_cast<T*>(g.p);
}

// Scratch of the centroid ranking (rank_centroids) of a chunk of queries.  Three holders: a probe slot (nmn_ivf_search of a
// Flat index), the coded search's scratch, and the per-stream scratch of nmn_ivf_search_device.
struct RankScratch {
    Grow qraw;          // the chunk's queries as the host passed them (dim floats each)
    Grow qpad;          // padded to the centroids' row stride (launch_qprep; not written where the raw queries serve)
    Grow qinfo;         // all zero while the queries are raw: zeroed whenever it is (re)allocated, written by launch_qprep only
    Grow qstate;
    Grow cscores;       // exact -d^2 of every query against every centroid (tile-major)
    Grow ckeys;         // sort buffer and scores of the large-k sort (more than kRankMax centroids only)
    Grow probe_rows;    // [query][n_clusters] clusters in probe order
    Grow probe_scores;
    Grow probe_rank;    // [query][n_clusters] probe rank or kNoRank
    Grow probe_count;
    template <class F>
    void for_each(F&& fn) {
        for (Grow* g : {&qraw, &qpad, &qinfo, &qstate, &cscores, &ckeys, &probe_rows, &probe_scores, &probe_rank, &probe_count}) fn(*g);
    }
    // sized for chunks of `nb` queries; stage: the queries come from the host and pass through qraw
    hipError_t reserve(const nmn_ivf* ivf, uint32_t nb, bool stage, hipStream_t s, bool& wait);
};

}  // namespace

struct nmn_ivf {
    nmn_index* vectors = nullptr;
    nmn_index* centroids = nullptr;
    uint32_t n_clusters = 0, dim = 0;
    int device = 0;
    uint64_t cap = 0;
    // The same vectors a second time in LIST-MAJOR order (the reference's IVFStorage::Flat keeps a Vec per list, ivf.rs:160-175):
    // the rows of list 0, then list 1, ..., ids ascending inside a list.  A probe over it reads contiguous row ranges instead of
    // a bitmap's worth of scattered rows, and no per-row side array at all.  Rebuilt (ivf_relayout) after a build / load and
    // when the vectors added since make up an eighth of it; those younger vectors are scanned in `vectors` through the bitmap.
    nmn_index* cvec = nullptr;
    uint64_t c_rows = 0;                 // ids [0, c_rows) are in cvec
    std::vector<uint32_t> perm_host;     // cvec row -> id
    std::vector<uint32_t> list_off_host; // [n_clusters + 1] first cvec row of every list
    uint32_t* list_off = nullptr;        // device copy
    bool cvec_failed = false;            // no HBM for the copy: probes stay on the bitmap over `vectors`
    uint32_t flags = 0, cand_cap = 0;    // of the nmn_index_desc the index was created with
    uint32_t* assign = nullptr;          // device [cap]
    std::vector<uint32_t> assign_host;   // same, for cluster_sizes and the tie order of equal distances
    std::vector<float> centroids_host;   // trained centroids (nmn_ivf_build), row-major n_clusters x dim
    hipStream_t stream = nullptr;
    uint32_t* cscores = nullptr;         // exact -d^2 of a chunk of queries vs every centroid (tile-major)
    size_t cscores_cap = 0;
    QInfo* qinfo = nullptr;              // [kAssignChunk] zeros (the assignment sweep's rows are padded queries as they are)
    uint32_t assign_chunk = kAssignChunk;
    // Searches hold `rw` shared (add / build / the accessors exclusive) and take a PROBE SLOT each: stream and scratch of
    // one centroid ranking + selection bitmap, created on demand.  The list scans themselves go through the flat index's
    // host API, whose coalescer lets several selective probes run side by side.
    std::shared_mutex rw;
    struct ProbeSlot {
        hipStream_t stream = nullptr;
        RankScratch rank;
        Grow mask;                       // selection over the id-ordered vectors, a bitmap per query of the chunk
        Grow mask_c;                     // selection over the list-major copy
        Grow pin{nullptr, 0, true};      // [queries nb x dim x 4 | probe rows nb x n_clusters x 8]
        uint32_t nb = 0;                 // queries of one chunk the buffers above are sized for (probe_slot_grow)
        // a lone query's list scans enqueued right behind its bitmaps (one round trip per call): their results, device and pinned,
        // two parts (list-major copy, younger vectors) of res_k entries each: [rows u64 | scores f32 | count u32]
        Grow res_dev, res_pin{nullptr, 0, true};
        uint64_t res_k = 0;
        bool busy = false;
        template <class F>
        void for_each(F&& fn) {
            rank.for_each(fn);
            for (Grow* g : {&mask, &mask_c, &pin, &res_dev, &res_pin}) fn(*g);
        }
    };
    std::vector<std::unique_ptr<ProbeSlot>> slots;
    std::mutex slot_mu;
    std::condition_variable slot_cv;
    std::vector<uint64_t> list_sizes;    // rows per cluster (host), for the selectivity hint of a probe
    uint64_t list_sizes_rows = 0;        // rows accounted for in list_sizes
    static constexpr size_t kMaxSlots = 64;
    // ---- IVF-PQ / IVF-Binary (kind != NMN_IVF_FLAT): `vectors` and `cvec` stay null, the lists hold codes -----------------
    int32_t kind = NMN_IVF_FLAT;
    uint32_t pq_m = 0, pq_k = 0, pq_sub = 0;  // subspaces, codewords per subspace (K'), subspace dimension
    int32_t bq_method = 0;                    // NMN_BINARY_*
    uint32_t code_bytes = 0;                  // per vector: M (PQ) or 8 * ceil(dim / 64) (Binary)
    uint64_t n_coded = 0, row_base = 0;       // vectors added; ids are row_base + [0, n_coded)
    std::vector<uint8_t> codes_host;          // id order (nmn_ivf_codes; the source of every re-layout)
    std::vector<float> codebook_host;         // [M][K'][pq_sub]
    float* codebook = nullptr;                // device copy
    uint8_t* lcodes = nullptr;                // device, LIST-MAJOR codes [cap][code_bytes] (order of perm_host)
    // one coded search at a time owns the scratch below (searches of a PQ / Binary index are serialised; `add` holds rw exclusively)
    std::mutex codec_mu;
    struct CodecScratch {
        RankScratch rank;
        Grow segs, base, tables, qwords, scores, keys, rows, rscores, rcnt;
        template <class F>
        void for_each(F&& fn) {
            rank.for_each(fn);
            for (Grow* g : {&segs, &base, &tables, &qwords, &scores, &keys, &rows, &rscores, &rcnt}) fn(*g);
        }
    } cs;
    // ---- nmn_ivf_search_device (docs/ivf.md §3.10c): a scratch of its own per caller stream, nothing of the probe slots or `cs` ----
    // The candidate-order id map of every storage: dev_perm[dev_off[c] + j] = id - id base of the j-th vector of list c (ids
    // ascending inside a list; for Flat over ALL the vectors, list-major copy and younger ones alike), built by the first
    // device search and again after an `add` (dev_gen != gen).  dev_top[i] = rows of the i largest lists (the host-known bound
    // of a query's candidates at nprobe i).
    std::mutex dev_mu;                   // the members below
    uint64_t gen = 0, dev_gen = ~0ull;   // gen: bumped by every add
    uint32_t* dev_perm = nullptr;
    uint32_t* dev_off = nullptr;
    uint64_t dev_rows = 0;
    std::vector<uint64_t> dev_top;
    struct DevScratch {                  // per caller stream: pipelined calls on one stream share it, in stream order
        hipStream_t stream = nullptr;
        std::mutex mu;                   // held while a call enqueues
        RankScratch rank;
        Grow segs, base, totals, scores, keys, tables, qwords;
        template <class F>
        void for_each(F&& fn) {
            rank.for_each(fn);
            for (Grow* g : {&segs, &base, &totals, &scores, &keys, &tables, &qwords}) fn(*g);
        }
    };
    std::vector<std::unique_ptr<DevScratch>> dev_scratch;
    // an event per device search, recorded behind its last kernel: add / destroy wait for the pending ones before they touch
    // what those searches read (completed events are recycled)
    std::vector<hipEvent_t> ev_pending, ev_free;
};

#define IVF_TRY(expr)                                         \
    do {                                                      \
        hipError_t _e = (expr);                               \
        if (_e != hipSuccess) return set_error_hip(_e, #expr); \
    } while (0)

// wait for the device searches still in flight (caller holds rw exclusively, or owns the index alone)
static void ivf_wait_device_searches(nmn_ivf* ivf) {
    std::lock_guard<std::mutex> lk(ivf->dev_mu);
    for (hipEvent_t e : ivf->ev_pending) {
        (void)hipEventSynchronize(e);
        ivf->ev_free.push_back(e);
    }
    ivf->ev_pending.clear();
}

extern "C" nmn_status nmn_ivf_destroy(nmn_ivf* ivf) {
    if (!ivf) return NMN_OK;
    (void)hipSetDevice(ivf->device);
    ivf_wait_device_searches(ivf);
    for (hipEvent_t e : ivf->ev_free) (void)hipEventDestroy(e);
    auto drop = [](Grow& g) { g.release(); };  // (nmn_ivf_hbm_bytes walks the same enumerators)
    for (auto& sc : ivf->dev_scratch) sc->for_each(drop);
    if (ivf->stream) (void)hipStreamSynchronize(ivf->stream);
    for (auto& sl : ivf->slots) {
        if (sl->stream) {
            (void)hipStreamSynchronize(sl->stream);
            (void)hipStreamDestroy(sl->stream);
        }
        sl->for_each(drop);
    }
    if (ivf->stream) (void)hipStreamDestroy(ivf->stream);
    ivf->cs.for_each(drop);
    for (void* p : {(void*)ivf->assign, (void*)ivf->cscores, (void*)ivf->qinfo, (void*)ivf->list_off, (void*)ivf->codebook,
                    (void*)ivf->lcodes, (void*)ivf->dev_perm, (void*)ivf->dev_off})
        if (p) (void)hipFree(p);
    if (ivf->cvec) nmn_index_destroy(ivf->cvec);
    if (ivf->vectors) nmn_index_destroy(ivf->vectors);
    if (ivf->centroids) nmn_index_destroy(ivf->centroids);
    delete ivf;
    return NMN_OK;
}

// allocate the index; `centroids` may be null (nmn_ivf_build trains them afterwards).  coded: a PQ / Binary index — no flat
// index of vectors (its lists hold codes, laid out by codec_layout), per-row device arrays sized by the codes instead.
static nmn_status ivf_new(const nmn_index_desc* desc, const float* centroids, uint32_t n_clusters, nmn_ivf** out, bool coded = false) {
    *out = nullptr;
    if (n_clusters == 0) return set_error(NMN_ERR_INVALID_ARGUMENT, "an IVF index needs at least one centroid");
    nmn_ivf* ivf = new (std::nothrow) nmn_ivf();
    if (!ivf) return set_error(NMN_ERR_OUT_OF_MEMORY, "host alloc");
    auto bail = [&](nmn_status st) {
        nmn_ivf_destroy(ivf);
        return st;
    };
    nmn_status st = NMN_OK;
    if (!coded) {
        st = nmn_index_create(desc, &ivf->vectors);
        if (st != NMN_OK) return bail(st);
    }
    nmn_index_desc cd = *desc;
    cd.capacity_rows = n_clusters;
    cd.row_base = 0;
    cd.device = coded ? desc->device : ivf->vectors->device;
    st = nmn_index_create(&cd, &ivf->centroids);
    if (st != NMN_OK) return bail(st);
    if (centroids) {
        st = nmn_index_upload(ivf->centroids, centroids, 0, n_clusters);
        if (st != NMN_OK) return bail(st);
    }
    ivf->n_clusters = n_clusters;
    ivf->flags = desc->flags;
    ivf->cand_cap = desc->cand_cap;
    ivf->dim = desc->dim;
    ivf->device = ivf->centroids->device;
    ivf->cap = coded ? desc->capacity_rows : ivf->vectors->cap;
    ivf->row_base = desc->row_base;
    const size_t c_pad = ivf->centroids->cap_pad;
    hipError_t e = hipSetDevice(ivf->device);
    auto alloc = [&](void** p, size_t bytes) {
        if (e == hipSuccess) e = hipMalloc(p, std::max<size_t>(bytes, 64));
    };
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&ivf->stream, hipStreamNonBlocking);
    alloc(reinterpret_cast<void**>(&ivf->assign), coded ? 64 : std::max<uint64_t>(ivf->cap, 1) * 4);
    // rows assigned per sweep: bound the score matrix to 64 MiB whatever the number of clusters
    ivf->assign_chunk = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(kAssignChunk, (16ull << 20) / c_pad));
    ivf->cscores_cap = c_pad * ivf->assign_chunk;
    alloc(reinterpret_cast<void**>(&ivf->cscores), ivf->cscores_cap * 4);
    alloc(reinterpret_cast<void**>(&ivf->qinfo), sizeof(QInfo) * kAssignChunk);
    if (e == hipSuccess) e = hipMemsetAsync(ivf->qinfo, 0, sizeof(QInfo) * kAssignChunk, ivf->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ivf->stream);
    if (e != hipSuccess) return bail(set_error_hip(e, "nmn_ivf_create"));
    *out = ivf;
    return NMN_OK;
}

extern "C" nmn_status nmn_ivf_create(const nmn_index_desc* desc, const float* centroids, uint32_t n_clusters,
                                     nmn_ivf** out) {
    if (!desc || !centroids || !out) return set_error(NMN_ERR_INVALID_ARGUMENT, "null argument");
    return ivf_new(desc, centroids, n_clusters, out);
}

extern "C" uint64_t nmn_ivf_len(const nmn_ivf* ivf) { return ivf ? (ivf->vectors ? ivf->vectors->rows : ivf->n_coded) : 0; }
extern "C" uint32_t nmn_ivf_clusters(const nmn_ivf* ivf) { return ivf ? ivf->n_clusters : 0; }
extern "C" nmn_index* nmn_ivf_vectors(nmn_ivf* ivf) { return ivf ? ivf->vectors : nullptr; }

extern "C" nmn_status nmn_ivf_cluster_sizes(nmn_ivf* ivf, uint64_t* out_sizes) {
    if (!ivf || !out_sizes) return set_error(NMN_ERR_INVALID_ARGUMENT, "null argument");
    std::unique_lock<std::shared_mutex> g(ivf->rw);
    std::fill(out_sizes, out_sizes + ivf->n_clusters, 0ull);
    for (uint32_t c : ivf->assign_host) out_sizes[c]++;
    return NMN_OK;
}

// The exact sweep every stage here is built on: scores (tile-major, score_at) = -d^2 of `nq` padded queries (device memory, stride
// x->ld; qinfo: zeros, or launch_qprep's) against rows [0, n_rows) of `x`.
static hipError_t sweep_neg_l2sq(const nmn_index* x, uint64_t n_rows, uint32_t dim, const float* qpad, const QInfo* qinfo, uint32_t nq,
                                 uint32_t* scores, hipStream_t s) {
    ExactScanParams ep{};
    ep.corpus = x->corpus;
    ep.norms = x->norms;
    ep.qpad = qpad;
    ep.qinfo = qinfo;
    ep.scores = scores;
    ep.n_rows = n_rows;
    ep.nql = nq;
    ep.ld = x->ld;
    ep.dim = dim;
    ep.nq = nq;
    ep.metric = kMetricNegL2Sq;
    return launch_exact_scan(ep, s);
}

// exact -d^2 of `nq` queries (already padded to ld in device memory) against every centroid -> cscores
static nmn_status centroid_scores(nmn_ivf* ivf, const float* qpad_dev, uint32_t nq) {
    IVF_TRY(sweep_neg_l2sq(ivf->centroids, ivf->n_clusters, ivf->dim, qpad_dev, ivf->qinfo, nq, ivf->cscores, ivf->stream));
    return NMN_OK;
}

// The raw queries ARE the padded ones where the rows are not padded (stride == dim) and the eight-lanes-per-row scan serves
// (fewer than 2^16 centroids): the centroid ranking is a squared-distance scan, it reads the first `dim` elements of each query and
// nothing qprep derives (no magnitude, no margins), so no qprep launch in front of it (5.6 us + a 4-us gap of a lone probe's ~150,
// profiles/r05q_*).  Constant for the life of an index.
static bool raw_queries(const nmn_ivf* ivf) {
    return ivf->centroids->ld == ivf->dim && (!ivf->vectors || ivf->vectors->ld == ivf->dim) && ivf->n_clusters < (1u << 16);
}

hipError_t RankScratch::reserve(const nmn_ivf* ivf, uint32_t nb, bool stage, hipStream_t s, bool& wait) {
    const size_t C = ivf->n_clusters, c_pad = ivf->centroids->cap_pad, ld = ivf->centroids->ld, qinfo_cap = qinfo.cap;
    hipError_t e = hipSuccess;
    auto need = [&](Grow& g, size_t bytes) {
        if (e == hipSuccess) e = g.reserve(bytes, s, wait);
    };
    if (stage) need(qraw, (size_t)ivf->dim * nb * 4);
    need(qpad, ld * nb * 4);
    need(qinfo, sizeof(QInfo) * nb);
    need(qstate, sizeof(QState) * nb);
    need(cscores, c_pad * nb * 4);
    need(probe_rows, C * nb * 8);
    need(probe_rank, C * nb * 4);
    need(probe_count, (size_t)nb * 8);
    if (C > kRankMax) {  // the large-k sort, one query at a time
        need(ckeys, largek_sort_len(C) * 8);
        need(probe_scores, C * 4);
    }
    if (e == hipSuccess && qinfo.cap != qinfo_cap) e = hipMemsetAsync(qinfo.p, 0, qinfo.cap, s);
    return e;
}

// Stage one of every search: the centroids of `nb` queries (device memory, dim floats each) ranked by squared distance, ascending,
// ties by centroid index; the first `np` kept.  Everything on `s`, nothing waited for.  Up to kRankMax centroids: query q's probe
// order at probe_rows + q * n_clusters, its ranks at probe_rank + q * n_clusters, its count at probe_count + q.  Above: nb == 1,
// the large-k sort writes probe_rows, probe_scores and probe_count; probe_rank only where the caller reads it (fill_rank).
static nmn_status rank_centroids(nmn_ivf* ivf, const float* queries_dev, uint32_t nb, uint32_t np, RankScratch& sc, bool fill_rank,
                                 hipStream_t s) {
    const uint32_t C = ivf->n_clusters;
    const bool raw_q = raw_queries(ivf);
    if (!raw_q)
        IVF_TRY(launch_qprep(queries_dev, nb, ivf->dim, ivf->centroids->ld, kMetricNegL2Sq, ivf->centroids->max_norm_bits, gp<float>(sc.qpad),
                             gp<QInfo>(sc.qinfo), gp<QState>(sc.qstate), 0, s));
    IVF_TRY(sweep_neg_l2sq(ivf->centroids, C, ivf->dim, raw_q ? queries_dev : gp<float>(sc.qpad), gp<QInfo>(sc.qinfo), nb,
                           gp<uint32_t>(sc.cscores), s));
    if (C <= kRankMax) {
        uint32_t np2 = 2;
        while (np2 < C) np2 <<= 1;
        hipLaunchKernelGGL(ivf_rank_kernel, dim3(nb), dim3(1024), 0, s, gp<uint32_t>(sc.cscores), nb, C, np2, np, gp<uint64_t>(sc.probe_rows),
                           gp<uint32_t>(sc.probe_count), gp<uint32_t>(sc.probe_rank));
    } else {
        IVF_TRY(launch_largek(gp<uint32_t>(sc.cscores), C, gp<uint64_t>(sc.ckeys), np, 0, gp<uint64_t>(sc.probe_rows), gp<float>(sc.probe_scores),
                              gp<uint32_t>(sc.probe_count), s));
        if (fill_rank) {
            IVF_TRY(hipMemsetAsync(sc.probe_rank.p, 0xFF, (size_t)C * 4, s));
            hipLaunchKernelGGL(ivf_probe_rank_kernel, dim3((np + 255) / 256), dim3(256), 0, s, gp<uint64_t>(sc.probe_rows),
                               gp<uint32_t>(sc.probe_count), gp<uint32_t>(sc.probe_rank));
        }
    }
    IVF_TRY(hipGetLastError());
    return NMN_OK;
}

// nearest centroid (first minimum of the exact squared distances) of rows [row0, row0 + n) -> assign / assign_host
static nmn_status assign_rows(nmn_ivf* ivf, uint64_t row0, uint64_t n) {
    const uint32_t ld = ivf->vectors->ld;
    if (ivf->assign_host.size() < row0 + n) ivf->assign_host.resize(row0 + n);
    for (uint64_t off = 0; off < n; off += ivf->assign_chunk) {
        const uint32_t cnt = (uint32_t)std::min<uint64_t>(ivf->assign_chunk, n - off);
        // the rows are laid out exactly like padded queries: score them against the centroids in place
        nmn_status st = centroid_scores(ivf, ivf->vectors->corpus + (row0 + off) * (uint64_t)ld, cnt);
        if (st != NMN_OK) return st;
        hipLaunchKernelGGL(ivf_assign_kernel, dim3((cnt * 64 + 255) / 256), dim3(256), 0, ivf->stream, ivf->cscores,
                           ivf->n_clusters, cnt, cnt, ivf->assign + row0 + off);
        IVF_TRY(hipGetLastError());
        IVF_TRY(hipMemcpyAsync(ivf->assign_host.data() + row0 + off, ivf->assign + row0 + off, (size_t)cnt * 4,
                               hipMemcpyDeviceToHost, ivf->stream));
    }
    IVF_TRY(hipStreamSynchronize(ivf->stream));
    if (row0 == 0 || ivf->list_sizes.size() != ivf->n_clusters) {
        ivf->list_sizes.assign(ivf->n_clusters, 0);
        for (uint64_t r = 0; r < row0; r++) ivf->list_sizes[ivf->assign_host[r]]++;
    }
    for (uint64_t r = row0; r < row0 + n; r++) ivf->list_sizes[ivf->assign_host[r]]++;
    ivf->list_sizes_rows = row0 + n;
    return NMN_OK;
}

// (Re)build the list-major copy from the id-ordered vectors and their list assignments.  Caller holds ivf->rw exclusively.
// A stable counting sort of the assignments gives the permutation; the rows are gathered on the device 128 Ki rows at a time
// and go through the ordinary device upload (magnitudes, mirrors).  Not enough HBM for the copy is not an error.
static nmn_status ivf_relayout(nmn_ivf* ivf) {
    static const bool disabled = getenv("NMN_IVF_NO_LIST_MAJOR") != nullptr;  // A/B: every probe through the bitmap over `vectors`
    const uint64_t n = ivf->vectors->rows;
    if (disabled || ivf->cvec_failed || n < 4096 || ivf->assign_host.size() < n) return NMN_OK;
    IVF_TRY(hipSetDevice(ivf->device));
    if (!ivf->cvec) {
        nmn_index_desc d{};
        d.dim = ivf->dim;
        d.flags = ivf->flags;
        d.capacity_rows = ivf->cap;
        d.row_base = 0;
        d.device = ivf->device;
        d.cand_cap = ivf->cand_cap;
        if (nmn_index_create(&d, &ivf->cvec) != NMN_OK || ivf->cvec->ld != ivf->vectors->ld) {
            if (ivf->cvec) nmn_index_destroy(ivf->cvec);
            ivf->cvec = nullptr;
            ivf->cvec_failed = true;
            ivf->c_rows = 0;
            return NMN_OK;
        }
    }
    const uint32_t C = ivf->n_clusters;
    ivf->list_off_host.assign((size_t)C + 1, 0u);
    for (uint64_t r = 0; r < n; r++) ivf->list_off_host[ivf->assign_host[r] + 1]++;
    for (uint32_t c = 0; c < C; c++) ivf->list_off_host[c + 1] += ivf->list_off_host[c];
    ivf->perm_host.resize(n);
    {
        std::vector<uint32_t> cur(ivf->list_off_host.begin(), ivf->list_off_host.end() - 1);
        for (uint64_t r = 0; r < n; r++) ivf->perm_host[cur[ivf->assign_host[r]]++] = (uint32_t)r;  // ids ascending inside a list
    }
    constexpr uint64_t kChunk = 128 * 1024;
    uint32_t* perm_dev = nullptr;
    float* tmp = nullptr;
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&perm_dev), n * 4);
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&tmp), std::min(kChunk, n) * (uint64_t)ivf->dim * 4);
    if (e == hipSuccess && !ivf->list_off) e = hipMalloc(reinterpret_cast<void**>(&ivf->list_off), ((size_t)C + 1) * 4);
    if (e == hipSuccess) e = hipMemcpyAsync(perm_dev, ivf->perm_host.data(), n * 4, hipMemcpyHostToDevice, ivf->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(ivf->list_off, ivf->list_off_host.data(), ((size_t)C + 1) * 4, hipMemcpyHostToDevice, ivf->stream);
    nmn_status st = NMN_OK;
    for (uint64_t pos0 = 0; pos0 < n && e == hipSuccess && st == NMN_OK; pos0 += kChunk) {
        const uint32_t cnt = (uint32_t)std::min(kChunk, n - pos0);
        hipLaunchKernelGGL(ivf_gather_kernel, dim3(std::min<uint32_t>(cnt, 4096)), dim3(256), 0, ivf->stream, ivf->vectors->corpus,
                           ivf->vectors->ld, ivf->dim, perm_dev, pos0, cnt, tmp);
        e = hipGetLastError();
        if (e == hipSuccess) st = nmn_index_upload_device(ivf->cvec, tmp, pos0, cnt, ivf->stream);
        if (e == hipSuccess && st == NMN_OK) e = hipStreamSynchronize(ivf->stream);  // (`tmp` is reused by the next chunk)
    }
    if (e == hipSuccess) e = hipStreamSynchronize(ivf->stream);
    if (perm_dev) (void)hipFree(perm_dev);
    if (tmp) (void)hipFree(tmp);
    if (e != hipSuccess || st != NMN_OK) {
        // (out of memory half way, ...): drop the copy, keep serving from the bitmap over `vectors`
        (void)hipGetLastError();
        nmn_index_destroy(ivf->cvec);
        ivf->cvec = nullptr;
        ivf->cvec_failed = true;
        ivf->c_rows = 0;
        return NMN_OK;
    }
    ivf->c_rows = n;
    return NMN_OK;
}

extern "C" uint64_t nmn_ivf_list_major_rows(const nmn_ivf* ivf) { return ivf ? ivf->c_rows : 0; }

static nmn_status codec_add(nmn_ivf* ivf, const float* rows_host, uint64_t n, uint32_t* clusters_out);

extern "C" nmn_status nmn_ivf_add(nmn_ivf* ivf, const float* rows_host, uint64_t n, uint32_t* clusters_out) {
    if (!ivf || (n && !rows_host)) return set_error(NMN_ERR_INVALID_ARGUMENT, "null argument");
    if (n == 0) return NMN_OK;
    std::unique_lock<std::shared_mutex> g(ivf->rw);
    // a device search answers for the index as it was when it was enqueued: let those in flight finish before anything they
    // read changes (the codes' re-layout rewrites lcodes in place), and have the next one rebuild its id map
    ivf_wait_device_searches(ivf);
    ivf->gen++;
    if (ivf->kind != NMN_IVF_FLAT) return codec_add(ivf, rows_host, n, clusters_out);
    const uint64_t row0 = ivf->vectors->rows;
    nmn_status st = nmn_index_upload(ivf->vectors, rows_host, row0, n);  // ids = insertion order (ivf.rs:287-289)
    if (st != NMN_OK) return st;
    IVF_TRY(hipSetDevice(ivf->device));
    IVF_TRY(hipStreamSynchronize(ivf->vectors->host_stream));  // rows are in place before another stream reads them
    st = assign_rows(ivf, row0, n);
    if (st != NMN_OK) return st;
    if (clusters_out) memcpy(clusters_out, ivf->assign_host.data() + row0, n * 4);
    // the vectors added since the list-major copy was laid out are scanned through the bitmap; once they are an eighth of it
    // (or there is no copy yet and the index is worth one) it is laid out afresh
    const uint64_t rows = row0 + n, young = rows - ivf->c_rows;
    if (young >= std::max<uint64_t>(4096, ivf->c_rows / 8)) return ivf_relayout(ivf);
    return NMN_OK;
}

// ---- IVFIndex::train + add on the GPU (ivf.rs:222-316; KMeans::fit, delta_vector.rs:737-901) ----------------------
namespace {

inline uint64_t lcg(uint64_t s) { return s * 6364136223846793005ull + 1ull; }  // wrapping_mul / wrapping_add

// euclidean_distance_sq (delta_vector.rs:896-901) on the host: k * dim per iteration (centroid movement only)
float host_dist_sq(const float* a, const float* b, uint64_t dim) {
    float s = -0.0f;
    for (uint64_t i = 0; i < dim; i++) {
        const float d = a[i] - b[i];
        const float p = d * d;
        s = s + p;
    }
    return s;
}

}  // namespace

// IVFIndex::train + add for IVFStorage::Flat; layout = false leaves out the list-major copy (a PQ / Binary build and the
// codebook's per-subspace k-means only need the centroids and the assignments of this index, then destroy it)
static nmn_status ivf_train_flat(const nmn_index_desc* desc, const float* rows_host, uint64_t n, uint32_t num_clusters,
                                 const nmn_kmeans_options* opt, bool layout, nmn_ivf** out) {
    if (!desc || !rows_host || !opt || !out) return set_error(NMN_ERR_INVALID_ARGUMENT, "null argument");
    *out = nullptr;
    if (n == 0 || num_clusters == 0) return set_error(NMN_ERR_INVALID_ARGUMENT, "nothing to train on");
    if (desc->capacity_rows < n) return set_error(NMN_ERR_CAPACITY, "capacity_rows < n");
    const uint32_t k = (uint32_t)std::min<uint64_t>(num_clusters, n);  // `k.min(vectors.len())`
    const uint64_t dim = desc->dim;
    nmn_ivf* ivf = nullptr;
    nmn_status st = ivf_new(desc, nullptr, k, &ivf);
    if (st != NMN_OK) return st;
    auto bail = [&](nmn_status code) {
        nmn_ivf_destroy(ivf);
        return code;
    };
    std::unique_lock<std::shared_mutex> g(ivf->rw);
    st = nmn_index_upload(ivf->vectors, rows_host, 0, n);  // ids = order of the input (ivf.rs:287-289)
    if (st != NMN_OK) return bail(st);
    hipError_t he = hipSetDevice(ivf->device);
    if (he == hipSuccess) he = hipStreamSynchronize(ivf->vectors->host_stream);
    if (he != hipSuccess) return bail(set_error_hip(he, "nmn_ivf_build"));
    const uint32_t ld = ivf->vectors->ld;
    hipStream_t s = ivf->stream;
    std::vector<float> cents((size_t)k * dim);  // current centroids, host copy (row-major k x dim)

    // ---- initialisation -----------------------------------------------------------------------------------
    if (opt->init_method == 0) {  // KMeansInit::Random: Fisher-Yates with the LCG, first k indices (delta_vector.rs:781-800)
        std::vector<uint64_t> idx(n);
        for (uint64_t i = 0; i < n; i++) idx[i] = i;
        uint64_t state = opt->seed;
        for (uint64_t i = n - 1; i >= 1; i--) {
            state = lcg(state);
            std::swap(idx[i], idx[state % (i + 1)]);
        }
        for (uint32_t j = 0; j < k; j++) memcpy(cents.data() + (size_t)j * dim, rows_host + idx[j] * dim, dim * sizeof(float));
    } else {  // KMeansPlusPlus (delta_vector.rs:805-853): distances on the GPU, the f32 running sums on the host
        uint32_t* sweep = nullptr;
        float* dist_dev = nullptr;
        const uint64_t n_pad = (n + 63) & ~63ull;
        he = hipMalloc(reinterpret_cast<void**>(&sweep), n_pad * 4);
        if (he == hipSuccess) he = hipMalloc(reinterpret_cast<void**>(&dist_dev), n * 4);
        std::vector<float> dist(n, 3.402823466e+38f);  // f32::MAX
        if (he == hipSuccess) he = hipMemcpyAsync(dist_dev, dist.data(), n * 4, hipMemcpyHostToDevice, s);
        uint64_t state = lcg(opt->seed);
        uint64_t pick = state % n;
        memcpy(cents.data(), rows_host + pick * dim, dim * sizeof(float));
        for (uint32_t j = 1; j < k && he == hipSuccess; j++) {
            // dist[i] = min(dist[i], |v_i - last centroid|^2): the last centroid is row `pick`, already a padded query
            he = sweep_neg_l2sq(ivf->vectors, n, (uint32_t)dim, ivf->vectors->corpus + pick * (uint64_t)ld, ivf->qinfo, 1, sweep, s);
            if (he == hipSuccess) he = launch_kmeans_min_update(dist_dev, sweep, n, s);
            if (he == hipSuccess) he = hipMemcpyAsync(dist.data(), dist_dev, n * 4, hipMemcpyDeviceToHost, s);
            if (he == hipSuccess) he = hipStreamSynchronize(s);
            if (he != hipSuccess) break;
            float total = -0.0f;  // `distances.iter().sum()`
            for (uint64_t i = 0; i < n; i++) total = total + dist[i];
            state = lcg(state);
            if (total == 0.0f) {
                pick = state % n;
            } else {
                const float frac = (float)state / (float)UINT64_MAX;  // `rng_state as f32 / u64::MAX as f32`
                const float threshold = frac * total;
                float cumulative = 0.0f;
                pick = 0;
                for (uint64_t i = 0; i < n; i++) {
                    cumulative = cumulative + dist[i];
                    if (cumulative >= threshold) {
                        pick = i;
                        break;
                    }
                }
            }
            memcpy(cents.data() + (size_t)j * dim, rows_host + pick * dim, dim * sizeof(float));
        }
        if (sweep) (void)hipFree(sweep);
        if (dist_dev) (void)hipFree(dist_dev);
        if (he != hipSuccess) return bail(set_error_hip(he, "k-means++ initialisation"));
    }

    // ---- Lloyd iterations ---------------------------------------------------------------------------------
    uint32_t* members_dev = nullptr;
    uint64_t* offsets_dev = nullptr;
    float* new_dev = nullptr;
    he = hipMalloc(reinterpret_cast<void**>(&members_dev), n * 4);
    if (he == hipSuccess) he = hipMalloc(reinterpret_cast<void**>(&offsets_dev), ((size_t)k + 1) * 8);
    if (he == hipSuccess) he = hipMalloc(reinterpret_cast<void**>(&new_dev), (size_t)k * ld * 4);
    auto free_tmp = [&] {
        for (void* p : {(void*)members_dev, (void*)offsets_dev, (void*)new_dev})
            if (p) (void)hipFree(p);
    };
    if (he != hipSuccess) {
        free_tmp();
        return bail(set_error_hip(he, "k-means buffers"));
    }
    std::vector<uint32_t> members(n);
    std::vector<uint64_t> offsets((size_t)k + 1);
    std::vector<float> new_pad((size_t)k * ld), new_cents((size_t)k * dim);
    st = nmn_index_upload(ivf->centroids, cents.data(), 0, k);
    for (uint64_t it = 0; it < opt->max_iterations && st == NMN_OK; it++) {
        he = hipStreamSynchronize(ivf->centroids->host_stream);
        if (he != hipSuccess) break;
        st = assign_rows(ivf, 0, n);  // nearest_centroid for every vector (delta_vector.rs:755-757)
        if (st != NMN_OK) break;
        // update_centroids (867-893): members of each cluster in vector order (stable counting sort)
        std::fill(offsets.begin(), offsets.end(), 0ull);
        for (uint64_t i = 0; i < n; i++) offsets[ivf->assign_host[i] + 1]++;
        for (uint32_t c = 0; c < k; c++) offsets[c + 1] += offsets[c];
        {
            std::vector<uint64_t> cur(offsets.begin(), offsets.end() - 1);
            for (uint64_t i = 0; i < n; i++) members[cur[ivf->assign_host[i]]++] = (uint32_t)i;
        }
        he = hipMemcpyAsync(members_dev, members.data(), n * 4, hipMemcpyHostToDevice, s);
        if (he == hipSuccess) he = hipMemcpyAsync(offsets_dev, offsets.data(), ((size_t)k + 1) * 8, hipMemcpyHostToDevice, s);
        if (he == hipSuccess) he = launch_kmeans_update(ivf->vectors->corpus, ld, (uint32_t)dim, members_dev, offsets_dev, k, new_dev, s);
        if (he == hipSuccess) he = hipMemcpyAsync(new_pad.data(), new_dev, (size_t)k * ld * 4, hipMemcpyDeviceToHost, s);
        if (he == hipSuccess) he = hipStreamSynchronize(s);
        if (he != hipSuccess) break;
        float movement = 0.0f;  // `.fold(0.0f32, f32::max)` of the centroid displacements (763-767)
        for (uint32_t c = 0; c < k; c++) {
            memcpy(new_cents.data() + (size_t)c * dim, new_pad.data() + (size_t)c * ld, dim * sizeof(float));
            movement = std::fmax(movement, std::sqrt(host_dist_sq(cents.data() + (size_t)c * dim, new_cents.data() + (size_t)c * dim, dim)));
        }
        cents.swap(new_cents);
        st = nmn_index_upload(ivf->centroids, cents.data(), 0, k);
        if (movement < opt->convergence_threshold) break;
    }
    free_tmp();
    if (he != hipSuccess) return bail(set_error_hip(he, "k-means iteration"));
    if (st != NMN_OK) return bail(st);
    // ---- `for vector in &vectors { index.add(vector) }` under the trained centroids --------------------------
    he = hipStreamSynchronize(ivf->centroids->host_stream);
    if (he != hipSuccess) return bail(set_error_hip(he, "nmn_ivf_build"));
    st = assign_rows(ivf, 0, n);
    if (st != NMN_OK) return bail(st);
    ivf->centroids_host = cents;
    st = layout ? ivf_relayout(ivf) : NMN_OK;
    if (st != NMN_OK) return bail(st);
    *out = ivf;
    return NMN_OK;
}

extern "C" nmn_status nmn_ivf_build(const nmn_index_desc* desc, const float* rows_host, uint64_t n, uint32_t num_clusters,
                                    const nmn_kmeans_options* opt, nmn_ivf** out) {
    return ivf_train_flat(desc, rows_host, n, num_clusters, opt, true, out);
}

extern "C" nmn_status nmn_ivf_centroids(nmn_ivf* ivf, float* out, uint64_t cap_floats) {
    if (!ivf || !out) return set_error(NMN_ERR_INVALID_ARGUMENT, "null argument");
    std::unique_lock<std::shared_mutex> g(ivf->rw);
    const uint64_t need = (uint64_t)ivf->n_clusters * ivf->dim;
    if (cap_floats < need) return set_error(NMN_ERR_BUFFER_TOO_SMALL, "centroid buffer too small");
    if (ivf->centroids_host.size() == need) {
        memcpy(out, ivf->centroids_host.data(), need * sizeof(float));
        return NMN_OK;
    }
    IVF_TRY(hipSetDevice(ivf->device));
    IVF_TRY(hipMemcpy2D(out, (size_t)ivf->dim * 4, ivf->centroids->corpus, (size_t)ivf->centroids->ld * 4, (size_t)ivf->dim * 4,
                        ivf->n_clusters, hipMemcpyDeviceToHost));
    return NMN_OK;
}

// Size a slot's per-query buffers for chunks of `nb` queries (many queries of one nmn_ivf_search call share the centroid
// sweep, the ranking launch, the bitmap launches and ONE round trip to the host).  Only grows.
static nmn_status probe_slot_grow(nmn_ivf* ivf, nmn_ivf::ProbeSlot* sl, uint32_t nb) {
    if (nb <= sl->nb) return NMN_OK;
    const size_t C = ivf->n_clusters, words = (ivf->cap + 63) / 64 + 1;
    bool wait = sl->nb != 0;  // (nothing is enqueued on a slot just created, nor since a growth that failed: that one had waited)
    hipError_t e = sl->rank.reserve(ivf, nb, true, sl->stream, wait);
    if (e == hipSuccess) e = sl->mask.reserve(words * nb * 8, sl->stream, wait);
    if (e == hipSuccess) e = sl->mask_c.reserve(words * nb * 8, sl->stream, wait);
    if (e == hipSuccess) e = sl->pin.reserve((((size_t)ivf->dim * 4 * nb + 15) & ~(size_t)15) + C * 8 * nb + 16, sl->stream, wait);
    if (e != hipSuccess) {
        sl->nb = 0;  // (buffers in an unknown state: the next call grows them again from scratch)
        return set_error_hip(e, "IVF probe slot (chunk buffers)");
    }
    sl->nb = nb;
    return NMN_OK;
}

// a free probe slot (created on demand; waits when kMaxSlots are all busy)
static nmn_status probe_slot_acquire(nmn_ivf* ivf, nmn_ivf::ProbeSlot** out, uint32_t* busy_now = nullptr) {
    std::unique_lock<std::mutex> lk(ivf->slot_mu);
    if (busy_now) {
        *busy_now = 1;
        for (auto& sl : ivf->slots) *busy_now += sl->busy ? 1u : 0u;
    }
    for (;;) {
        for (auto& sl : ivf->slots)
            if (!sl->busy) {
                sl->busy = true;
                *out = sl.get();
                return NMN_OK;
            }
        if (ivf->slots.size() < nmn_ivf::kMaxSlots) break;
        ivf->slot_cv.wait(lk);
    }
    auto sl = std::make_unique<nmn_ivf::ProbeSlot>();
    hipError_t e = hipStreamCreateWithFlags(&sl->stream, hipStreamNonBlocking);
    nmn_status st = e == hipSuccess ? probe_slot_grow(ivf, sl.get(), 1) : set_error_hip(e, "IVF probe slot");
    if (st != NMN_OK) {
        if (sl->stream) (void)hipStreamDestroy(sl->stream);
        sl->for_each([](Grow& g) { g.release(); });
        return st;
    }
    sl->busy = true;
    *out = sl.get();
    ivf->slots.push_back(std::move(sl));
    return NMN_OK;
}

static void probe_slot_release(nmn_ivf* ivf, nmn_ivf::ProbeSlot* sl) {
    {
        std::lock_guard<std::mutex> g(ivf->slot_mu);
        sl->busy = false;
    }
    ivf->slot_cv.notify_one();
}

static nmn_status codec_search(nmn_ivf* ivf, const float* queries, uint32_t nq, uint32_t k, uint32_t nprobe, uint64_t* out_ids,
                               float* out_distances, uint32_t* out_counts);

extern "C" nmn_status nmn_ivf_search(nmn_ivf* ivf, const float* queries, uint32_t nq, uint32_t k, uint32_t nprobe,
                                     uint64_t* out_ids, float* out_distances, uint32_t* out_counts,
                                     nmn_search_stats* stats) {
    if (!ivf || !queries || !out_ids || !out_distances || !out_counts)
        return set_error(NMN_ERR_INVALID_ARGUMENT, "null argument");
    if (k == 0) return set_error(NMN_ERR_INVALID_TOP_K, "k == 0");
    if (nq == 0) return NMN_OK;
    std::shared_lock<std::shared_mutex> g(ivf->rw);  // concurrent with other searches, not with add / build
    if (ivf->kind != NMN_IVF_FLAT) {
        if (stats) memset(stats, 0, sizeof *stats);
        return codec_search(ivf, queries, nq, k, nprobe, out_ids, out_distances, out_counts);
    }
    IVF_TRY(hipSetDevice(ivf->device));
    const uint64_t n_rows = ivf->vectors->rows;
    const uint32_t np = std::min<uint32_t>(nprobe, ivf->n_clusters);  // ivf.rs:339
    std::vector<uint32_t> rank_host;
    std::vector<uint64_t> tmp_ids;
    std::vector<float> tmp_dist;
    nmn_ivf::ProbeSlot* sl = nullptr;
    uint32_t searches_now = 1;  // searches of this index in flight, this one included
    nmn_status st = probe_slot_acquire(ivf, &sl, &searches_now);
    if (st != NMN_OK) return st;
    struct Release {
        nmn_ivf* ivf;
        nmn_ivf::ProbeSlot* sl;
        ~Release() { probe_slot_release(ivf, sl); }
    } release{ivf, sl};
    hipStream_t s = sl->stream;
    // Queries are served in chunks of up to kProbeChunk: ONE copy of the chunk's queries, one exact sweep of all of them
    // over the centroids, one ranking launch (a workgroup per query), one launch per bitmap kind (a grid row per query) and
    // one copy of the probe orders back — a single round trip to the host for the whole chunk where every query used to pay
    // its own; the list scans then follow query by query (each its own bitmap and, with k + 1, its own tie handling).
    // (chunk: up to 64 queries, fewer when their bitmaps — two per query — would take more than 256 MiB)
    const size_t mask_words = (ivf->cap + 63) / 64 + 1;
    const uint32_t kProbeChunk = (uint32_t)std::max<size_t>(1, std::min<size_t>(64, ((size_t)256 << 20) / (mask_words * 16)));
    const uint32_t chunk = (ivf->n_clusters <= kRankMax) ? std::min<uint32_t>(nq, kProbeChunk) : 1u;  // (> 4096 lists: the large-k sort, one query at a time)
    st = probe_slot_grow(ivf, sl, chunk);
    if (st != NMN_OK) return st;
    float* pin_q = gp<float>(sl->pin);
    uint64_t* probe_host_all = reinterpret_cast<uint64_t*>(gp<uint8_t>(sl->pin) + (((size_t)ivf->dim * 4 * sl->nb + 15) & ~(size_t)15));
    float* const qraw = gp<float>(sl->rank.qraw);
    const uint64_t* const probe_rows = gp<uint64_t>(sl->rank.probe_rows);
    const uint32_t* const probe_rank = gp<uint32_t>(sl->rank.probe_rank);
    uint64_t* const mask = gp<uint64_t>(sl->mask);
    uint64_t* const mask_c = gp<uint64_t>(sl->mask_c);
    const uint64_t c_rows = ivf->cvec ? std::min(ivf->c_rows, n_rows) : 0;  // ids the list-major copy covers
    // The list scans of a chunk as ONE batch per part (list-major copy / younger vectors): the flat index's batched sweep reads a
    // bitmap per query, so sixteen probes cost one pass over the vectors instead of sixteen launch-bound searches — whenever that
    // pass is the cheaper way (the coalescer's own estimate: a search alone costs max(100 us, its share of a sweep)).
    const uint64_t kk1 = std::min<uint64_t>((uint64_t)k + 1, std::max<uint64_t>(n_rows, 1));
    std::vector<uint64_t> bc_ids, bt_ids, hint_c, hint_t;
    std::vector<float> bc_dist, bt_dist;
    std::vector<uint32_t> bc_cnt, bt_cnt;
    bool batched_c = false, batched_t = false;
    auto probed_of = [&](const uint64_t* probe_host, uint64_t* pc, uint64_t* pt) {
        uint64_t probed_rows = 0, probed_c = 0;
        for (uint32_t i = 0; i < np; i++)
            if (probe_host[i] < ivf->list_sizes.size()) {
                probed_rows += ivf->list_sizes[probe_host[i]];
                if (c_rows) probed_c += ivf->list_off_host[probe_host[i] + 1] - ivf->list_off_host[probe_host[i]];
            }
        if (ivf->list_sizes_rows != n_rows) probed_rows = UINT64_MAX;  // sizes not current (never after add / build)
        *pc = probed_c;
        *pt = (probed_rows == UINT64_MAX) ? UINT64_MAX : probed_rows - std::min(probed_rows, probed_c);
    };
    auto scan_many = [&](nmn_index* ix, const uint64_t* masks, const std::vector<uint64_t>& hints, const float* q0, uint32_t nb,
                         std::vector<uint64_t>& ids, std::vector<float>& dist, std::vector<uint32_t>& cnt, bool* done,
                         nmn_search_stats* stats_out) -> nmn_status {
        *done = false;
        static const bool no_many = getenv("NMN_IVF_NO_BATCHED_SCANS") != nullptr;  // (A/B switch)
        if (no_many || nb < 2 || kk1 > NMN_MAX_TOP_K || nb > index_hostio_many_capacity(ix, kMetricNegL2, (uint32_t)kk1)) return NMN_OK;
        const double sweep_us = (double)ix->rows * ix->ld * 2.0 / 5.5e6, fixed_us = 100.0;
        double separately = 0.0;
        for (uint32_t i = 0; i < nb; i++) {
            const double sel = hints[i] == UINT64_MAX ? 1.0 : (double)hints[i] / (double)std::max<uint64_t>(ix->rows, 1);
            separately += std::max(fixed_us, sel * sweep_us);
        }
        if (separately < 1.1 * sweep_us + fixed_us) return NMN_OK;
        ids.assign((size_t)nb * kk1, UINT64_MAX);
        dist.assign((size_t)nb * kk1, 0.f);
        cnt.assign(nb, 0);
        std::vector<HostSearchSpec> specs(nb);
        for (uint32_t i = 0; i < nb; i++) {
            specs[i].query = q0 + (size_t)i * ivf->dim;
            specs[i].mask = masks + (size_t)i * mask_words;
            specs[i].mask_rows = hints[i];
            specs[i].out_rows = ids.data() + (size_t)i * kk1;
            specs[i].out_scores = dist.data() + (size_t)i * kk1;
            specs[i].out_count = cnt.data() + i;
        }
        nmn_status st2 = index_search_hostio_many(ix, specs.data(), nb, (uint32_t)kk1, kMetricNegL2, stats_out);
        if (st2 == NMN_OK) *done = true;
        return st2;
    };
    for (uint32_t q = 0; q < nq; q++) {
        uint64_t* o_ids = out_ids + (size_t)q * k;
        float* o_dist = out_distances + (size_t)q * k;
        std::fill(o_ids, o_ids + k, UINT64_MAX);
        std::fill(o_dist, o_dist + k, __builtin_inff());
        out_counts[q] = 0;
        if (n_rows == 0 || np == 0) continue;
        const float* qh = queries + (size_t)q * ivf->dim;
        const uint32_t qc = q % chunk;  // position in its chunk
        if (qc == 0) {
            // 1. (whole chunk) rank the centroids by squared distance (ascending; ties by index), keep the first nprobe, turn the
            //    list assignments into selection bitmaps — all on this slot's stream, one wait
            const uint32_t nb = std::min<uint32_t>(chunk, nq - q);
            memcpy(pin_q, qh, (size_t)ivf->dim * 4 * nb);
            IVF_TRY(hipMemcpyAsync(qraw, pin_q, (size_t)ivf->dim * 4 * nb, hipMemcpyHostToDevice, s));
            st = rank_centroids(ivf, qraw, nb, np, sl->rank, true, s);  // (the bitmaps below read the ranks: above kRankMax too)
            if (st != NMN_OK) return st;
            if (c_rows) {
                const uint64_t cw = (c_rows + 63) / 64;
                hipLaunchKernelGGL(ivf_range_mask_kernel, dim3((uint32_t)std::min<uint64_t>((cw + 3) / 4, 4096), nb), dim3(256), 0, s,
                                   ivf->list_off, ivf->n_clusters, probe_rank, c_rows, mask_c, (uint64_t)mask_words);
            }
            if (c_rows < n_rows) {
                const uint64_t n_words = (n_rows + 63) / 64;
                const uint32_t blocks = (uint32_t)std::min<uint64_t>((n_words + 3) / 4, 4096);
                hipLaunchKernelGGL(ivf_mask_kernel, dim3(blocks, nb), dim3(256), 0, s, ivf->assign, probe_rank, ivf->n_clusters, n_rows,
                                   c_rows, mask, (uint64_t)mask_words);
            }
            IVF_TRY(hipGetLastError());
            // A lone query, nobody else searching: its list scans are enqueued HERE, on this stream, behind the bitmaps they read —
            // the probe order, both result lists and the counts come back in one copy each behind ONE wait (the call used to be two
            // round trips: 0.235 ms at 2M x 768 of which the scans' kernels are a third).  With other searches in flight the scans
            // go through the flat index's host path below instead, where the coalescer merges concurrent probes into batched sweeps.
            static const bool no_direct = getenv("NMN_IVF_NO_DIRECT") != nullptr;  // (A/B switch)
            const bool direct = nb == 1 && nq == 1 && searches_now <= 1 && !no_direct && kk1 <= NMN_MAX_TOP_K;
            const size_t part_bytes = ((size_t)kk1 * 12 + 4 + 15) & ~(size_t)15;
            if (direct) {
                if (sl->res_k < kk1) {
                    sl->res_k = 0;
                    bool wait = true;
                    IVF_TRY(sl->res_dev.reserve(2 * part_bytes, s, wait));
                    IVF_TRY(sl->res_pin.reserve(2 * part_bytes, s, wait));
                    sl->res_k = kk1;
                }
                uint8_t* const res_dev = gp<uint8_t>(sl->res_dev);
                const uint8_t* const res_pin = gp<uint8_t>(sl->res_pin);
                const size_t pb = (((size_t)sl->res_k * 12 + 4 + 15) & ~(size_t)15);
                auto part = [&](uint8_t* base, int i, uint64_t** r, float** sc, uint32_t** c) {
                    uint8_t* b = base + (size_t)i * pb;
                    *r = reinterpret_cast<uint64_t*>(b);
                    *sc = reinterpret_cast<float*>(b + (size_t)sl->res_k * 8);
                    *c = reinterpret_cast<uint32_t*>(b + (size_t)sl->res_k * 12);
                };
                // (this call waits for its answer: the list scans take the SHORT launch chain, nmn_index.h — a scan whose candidate
                //  list overflowed reports it in its count and is repeated below with the whole chain)
                auto enqueue_scans = [&](bool short_chain, bool want_c, bool want_t) -> nmn_status {
                    uint64_t* r;
                    float* sc;
                    uint32_t* c;
                    nmn_status e = NMN_OK;
                    if (c_rows && want_c) {
                        part(res_dev, 0, &r, &sc, &c);
                        e = index_search_device(ivf->cvec, qraw, 1, (uint32_t)kk1, kMetricNegL2, mask_c, r, sc, c, s, short_chain);
                        if (e != NMN_OK) return e;
                    }
                    if (c_rows < n_rows && want_t) {
                        part(res_dev, 1, &r, &sc, &c);
                        e = index_search_device(ivf->vectors, qraw, 1, (uint32_t)kk1, kMetricNegL2, mask, r, sc, c, s, short_chain);
                        if (e != NMN_OK) return e;
                    }
                    if (hipMemcpyAsync(sl->res_pin.p, res_dev, 2 * pb, hipMemcpyDeviceToHost, s) != hipSuccess)
                        return set_error(NMN_ERR_STORAGE, "ivf: result copy");
                    return NMN_OK;
                };
                st = enqueue_scans(true, true, true);
                if (st != NMN_OK) return st;
                IVF_TRY(hipMemcpyAsync(probe_host_all, probe_rows, (size_t)nb * ivf->n_clusters * 8, hipMemcpyDeviceToHost, s));
                IVF_TRY(hipStreamSynchronize(s));
                auto flagged = [&](int i) { return *reinterpret_cast<const uint32_t*>(res_pin + (size_t)i * pb + (size_t)sl->res_k * 12) == 0xFFFFFFFFu; };
                const bool again_c = c_rows && flagged(0), again_t = c_rows < n_rows && flagged(1);
                if (again_c || again_t) {
                    if (again_c) index_short_chain_flagged(ivf->cvec);
                    if (again_t) index_short_chain_flagged(ivf->vectors);
                    st = enqueue_scans(false, again_c, again_t);
                    if (st != NMN_OK) return st;
                    IVF_TRY(hipStreamSynchronize(s));
                }
            } else {
                IVF_TRY(hipMemcpyAsync(probe_host_all, probe_rows, (size_t)nb * ivf->n_clusters * 8, hipMemcpyDeviceToHost, s));
                IVF_TRY(hipStreamSynchronize(s));
            }
            if (direct) {
                const size_t pb = (((size_t)sl->res_k * 12 + 4 + 15) & ~(size_t)15);
                auto take = [&](int i, std::vector<uint64_t>& ids, std::vector<float>& dist, std::vector<uint32_t>& cnt) {
                    const uint8_t* b = gp<uint8_t>(sl->res_pin) + (size_t)i * pb;
                    const uint64_t* r = reinterpret_cast<const uint64_t*>(b);
                    const float* sc = reinterpret_cast<const float*>(b + (size_t)sl->res_k * 8);
                    ids.assign(r, r + kk1);
                    dist.assign(sc, sc + kk1);
                    cnt.assign(1, std::min<uint32_t>(*reinterpret_cast<const uint32_t*>(b + (size_t)sl->res_k * 12), (uint32_t)kk1));
                };
                batched_c = batched_t = false;
                if (c_rows) {
                    take(0, bc_ids, bc_dist, bc_cnt);
                    batched_c = true;
                }
                if (c_rows < n_rows) {
                    take(1, bt_ids, bt_dist, bt_cnt);
                    batched_t = true;
                }
                if (stats) {  // (what the host path reports for the last list scan of a call)
                    st = nmn_index_last_stats(c_rows ? ivf->cvec : ivf->vectors, s, stats);
                    if (st != NMN_OK) return st;
                }
            }
            // 2a. the chunk's list scans, batched where that pays (results at k + 1, picked up query by query below)
            hint_c.assign(nb, 0);
            hint_t.assign(nb, 0);
            for (uint32_t i = 0; i < nb; i++) probed_of(probe_host_all + (size_t)i * ivf->n_clusters, &hint_c[i], &hint_t[i]);
            if (!direct) batched_c = batched_t = false;
            if (c_rows && !direct) {
                st = scan_many(ivf->cvec, mask_c, hint_c, qh, nb, bc_ids, bc_dist, bc_cnt, &batched_c, (stats && q + nb == nq) ? stats : nullptr);
                if (st != NMN_OK) return st;
            }
            if (c_rows < n_rows && !direct) {
                st = scan_many(ivf->vectors, mask, hint_t, qh, nb, bt_ids, bt_dist, bt_cnt, &batched_t,
                               (stats && q + nb == nq && !c_rows) ? stats : nullptr);
                if (st != NMN_OK) return st;
            }
        }
        const uint64_t* probe_host = probe_host_all + (size_t)qc * ivf->n_clusters;
        const uint64_t* mask_q = mask + (size_t)qc * mask_words;
        const uint64_t* mask_cq = mask_c + (size_t)qc * mask_words;
        // rows in the probed lists: the selectivity hint of the list scan (how the flat index's coalescer decides what may
        // run side by side) and the most the scan can return
        uint64_t probed_c = 0, probed_t = 0;
        probed_of(probe_host, &probed_c, &probed_t);
        // 2. masked scan ranking by distance (negated so that nearest = largest).  One result more than asked for: the scan
        //    breaks equal distances by id, the reference by candidate order, so a run of equal distances that straddles
        //    the cut must be seen whole before it is reordered and cut.
        uint64_t kk = kk1;
        uint32_t cnt = 0;
        std::vector<uint64_t> part_ids;
        std::vector<float> part_dist;
        for (;;) {
            const bool first = kk == kk1;  // (the batched scans of 2a answer the first round; an extension searches alone)
            tmp_ids.assign(kk, UINT64_MAX);
            tmp_dist.assign(kk, 0.f);
            if (c_rows) {  // the list-major copy: results are ITS rows, mapped back to ids
                if (first && batched_c) {
                    cnt = bc_cnt[qc];
                    std::copy(bc_ids.begin() + (size_t)qc * kk1, bc_ids.begin() + (size_t)(qc + 1) * kk1, tmp_ids.begin());
                    std::copy(bc_dist.begin() + (size_t)qc * kk1, bc_dist.begin() + (size_t)(qc + 1) * kk1, tmp_dist.begin());
                } else {
                    st = index_search_hostio(ivf->cvec, qh, 1, (uint32_t)kk, kMetricNegL2, mask_cq, true, tmp_ids.data(), tmp_dist.data(),
                                             &cnt, (stats && q + 1 == nq) ? stats : nullptr, probed_c);
                    if (st != NMN_OK) return st;
                }
                for (uint32_t i = 0; i < cnt; i++) tmp_ids[i] = ivf->vectors->row_base + ivf->perm_host[tmp_ids[i]];
            }
            if (c_rows < n_rows) {  // the younger vectors, in id order
                uint32_t cnt_t = 0;
                part_ids.assign(kk, UINT64_MAX);
                part_dist.assign(kk, 0.f);
                if (first && batched_t) {
                    cnt_t = bt_cnt[qc];
                    std::copy(bt_ids.begin() + (size_t)qc * kk1, bt_ids.begin() + (size_t)(qc + 1) * kk1, part_ids.begin());
                    std::copy(bt_dist.begin() + (size_t)qc * kk1, bt_dist.begin() + (size_t)(qc + 1) * kk1, part_dist.begin());
                } else {
                    st = index_search_hostio(ivf->vectors, qh, 1, (uint32_t)kk, kMetricNegL2, mask_q, true, part_ids.data(), part_dist.data(),
                                             &cnt_t, (stats && q + 1 == nq && !c_rows) ? stats : nullptr, probed_t);
                    if (st != NMN_OK) return st;
                }
                if (!c_rows) {
                    tmp_ids.swap(part_ids);
                    tmp_dist.swap(part_dist);
                    cnt = cnt_t;
                } else if (cnt_t) {
                    // merge the two lists (each best first: score = -distance descending, ties by id) and keep kk
                    std::vector<uint64_t> mi(kk, UINT64_MAX);
                    std::vector<float> md(kk, 0.f);
                    uint32_t a = 0, b = 0, o = 0;
                    while (o < kk && (a < cnt || b < cnt_t)) {
                        const bool take_a = b >= cnt_t || (a < cnt && (tmp_dist[a] > part_dist[b] || (tmp_dist[a] == part_dist[b] && tmp_ids[a] < part_ids[b])));
                        if (take_a) { mi[o] = tmp_ids[a]; md[o] = tmp_dist[a]; a++; }
                        else { mi[o] = part_ids[b]; md[o] = part_dist[b]; b++; }
                        o++;
                    }
                    tmp_ids.swap(mi);
                    tmp_dist.swap(md);
                    cnt = o;
                }
            }
            const bool cut_inside_run = cnt > k && tmp_dist[k] == tmp_dist[k - 1];
            // the run is seen whole as soon as it ENDS inside the fetched list (its last fetched entry differs from the
            // k-th); only a run that reaches the end of a full list may continue beyond it
            const bool run_ends_inside = cut_inside_run && tmp_dist[cnt - 1] != tmp_dist[k - 1];
            if (!cut_inside_run || run_ends_inside || cnt < kk || kk >= n_rows) break;  // nothing more to learn / fetch
            kk = std::min<uint64_t>(kk * 2, n_rows);
        }
        // (0 - score, not -score: the scan's keys hold a zero distance as +0.0 (score_to_key folds -0.0 into it), and the reference's
        //  distance of a vector from itself is +0.0, never -0.0 — tests/test_gpu_knobs.py compares the bits)
        for (uint32_t i = 0; i < cnt; i++) tmp_dist[i] = 0.0f - tmp_dist[i];
        // 3. equal distances keep candidate order: probe order of the cluster, then id (stable sort, ivf.rs:402)
        bool any_tie = false;
        for (uint32_t i = 1; i < cnt && !any_tie; i++) any_tie = tmp_dist[i] == tmp_dist[i - 1];
        if (any_tie) {
            rank_host.assign(ivf->n_clusters, kNoRank);
            for (uint32_t i = 0; i < np; i++)
                if (probe_host[i] < ivf->n_clusters) rank_host[probe_host[i]] = i;
            const uint64_t base = ivf->vectors->row_base;
            for (uint32_t a = 0; a < cnt;) {
                uint32_t b = a + 1;
                while (b < cnt && tmp_dist[b] == tmp_dist[a]) b++;
                if (b - a > 1)
                    std::sort(tmp_ids.begin() + a, tmp_ids.begin() + b, [&](uint64_t x, uint64_t y) {
                        const uint32_t rx = rank_host[ivf->assign_host[x - base]], ry = rank_host[ivf->assign_host[y - base]];
                        return rx != ry ? rx < ry : x < y;
                    });
                a = b;
            }
        }
        const uint32_t keep = std::min<uint32_t>(cnt, k);
        std::copy(tmp_ids.begin(), tmp_ids.begin() + keep, o_ids);
        std::copy(tmp_dist.begin(), tmp_dist.begin() + keep, o_dist);
        out_counts[q] = keep;
    }
    return NMN_OK;
}

// ---- IVF-PQ / IVF-Binary storage (ivf.rs:61-157, 222-406; pq.rs:114-430; binary_quantization.rs:27-155) --------------------
// Centroids and list assignment are IVF-Flat's (the same exact k-means, the same nearest-centroid sweep); what a list holds
// is codes: M bytes per vector (PQ, residual v - centroid[list] encoded against the codebook) or ceil(dim / 64) u64 words
// (Binary, v itself against its own threshold).  The device keeps the codes LIST-MAJOR (rows of list 0, then list 1, ..., ids
// ascending inside a list, `perm_host` maps back) plus the centroids and the codebook — no f32 vector after the build.
// The host keeps the codes in id order too (inspection, re-layout after `add`: a stable counting sort and one upload).
// A search: the centroid ranking exactly as Flat's (exact -d^2 sweep + ivf_rank_kernel, up to 64 queries per launch), the probe
// orders to the host (one wait), then per group of queries one scan launch over every probed list of every query
// (nmn_ivf_codec.hip) writing the negated distance of each candidate in candidate order, one large-k sort per query (score
// desc, candidate index asc = the reference's stable sort by distance, ivf.rs:402-404), and one copy back.
namespace {

size_t index_hbm_bytes(const nmn_index* x) {
    if (!x) return 0;
    size_t b = (size_t)x->cap_pad * x->ld * 4 + (size_t)x->cap_pad * 8;  // f32 rows, magnitudes and their inverses
    if (x->half) b += (size_t)x->cap_pad * x->ld * 2;
    if (x->q8) b += (size_t)x->cap_pad * x->ld + (size_t)x->cap_pad * 16;
    return b;
}

nmn_status check_storage(const nmn_ivf_storage* s, uint32_t dim) {
    if (s->kind == NMN_IVF_PQ) {
        if (s->pq_num_subspaces == 0 || dim % s->pq_num_subspaces != 0)
            return set_error(NMN_ERR_CONFIGURATION, "IVF-PQ: vector dimension must be divisible by num_subspaces");
        if ((size_t)dim * 4 > 64 * 1024)
            return set_error(NMN_ERR_CONFIGURATION, "IVF-PQ: dimensions above 16384 are not supported on the device");
        return NMN_OK;
    }
    if (s->kind == NMN_IVF_BINARY) {
        if (s->binary_threshold < NMN_BINARY_SIGN || s->binary_threshold > NMN_BINARY_MEDIAN)
            return set_error(NMN_ERR_CONFIGURATION, "IVF-Binary: unknown threshold method");
        return NMN_OK;
    }
    return set_error(NMN_ERR_CONFIGURATION, "unknown IVF storage kind");
}

// the coded index shell: centroids uploaded, storage parameters set, code buffers allocated for desc->capacity_rows
nmn_status codec_new(const nmn_index_desc* desc, const float* centroids, uint32_t C, const nmn_ivf_storage* s, const float* codebook,
                     uint32_t K, nmn_ivf** out) {
    nmn_ivf* ivf = nullptr;
    nmn_status st = ivf_new(desc, centroids, C, &ivf, true);
    if (st != NMN_OK) return st;
    ivf->kind = s->kind;
    ivf->centroids_host.assign(centroids, centroids + (size_t)C * desc->dim);
    if (s->kind == NMN_IVF_PQ) {
        ivf->pq_m = s->pq_num_subspaces;
        ivf->pq_sub = desc->dim / ivf->pq_m;
        ivf->pq_k = K;
        ivf->code_bytes = ivf->pq_m;
        const size_t cbn = (size_t)ivf->pq_m * K * ivf->pq_sub;
        if (cbn) ivf->codebook_host.assign(codebook, codebook + cbn);
    } else {
        ivf->bq_method = s->binary_threshold;
        ivf->code_bytes = 8 * ((desc->dim + 63) / 64);
    }
    hipError_t e = hipSetDevice(ivf->device);
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&ivf->codebook), std::max<size_t>(ivf->codebook_host.size() * 4, 64));
    if (e == hipSuccess && !ivf->codebook_host.empty())
        e = hipMemcpy(ivf->codebook, ivf->codebook_host.data(), ivf->codebook_host.size() * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess)
        e = hipMalloc(reinterpret_cast<void**>(&ivf->lcodes), std::max<size_t>((size_t)std::max<uint64_t>(ivf->cap, 1) * ivf->code_bytes, 64));
    if (e != hipSuccess) {
        nmn_ivf_destroy(ivf);
        return set_error_hip(e, "IVF code buffers");
    }
    ivf->list_sizes.assign(C, 0);
    *out = ivf;
    return NMN_OK;
}

// list-major codes from the id-ordered ones: stable counting sort of the assignments, one upload.  Caller holds rw exclusively.
nmn_status codec_layout(nmn_ivf* ivf) {
    const uint64_t n = ivf->n_coded;
    const uint32_t C = ivf->n_clusters, cb = ivf->code_bytes;
    ivf->list_off_host.assign((size_t)C + 1, 0u);
    for (uint64_t r = 0; r < n; r++) ivf->list_off_host[ivf->assign_host[r] + 1]++;
    for (uint32_t c = 0; c < C; c++) ivf->list_off_host[c + 1] += ivf->list_off_host[c];
    ivf->perm_host.resize(n);
    std::vector<uint8_t> lm((size_t)n * cb);
    {
        std::vector<uint32_t> cur(ivf->list_off_host.begin(), ivf->list_off_host.end() - 1);
        for (uint64_t r = 0; r < n; r++) {
            const uint32_t pos = cur[ivf->assign_host[r]]++;
            ivf->perm_host[pos] = (uint32_t)r;
            memcpy(lm.data() + (size_t)pos * cb, ivf->codes_host.data() + (size_t)r * cb, cb);
        }
    }
    IVF_TRY(hipSetDevice(ivf->device));
    if (n) IVF_TRY(hipMemcpy(ivf->lcodes, lm.data(), lm.size(), hipMemcpyHostToDevice));
    ivf->c_rows = n;
    ivf->list_sizes.assign(C, 0);
    for (uint32_t c = 0; c < C; c++) ivf->list_sizes[c] = ivf->list_off_host[c + 1] - ivf->list_off_host[c];
    ivf->list_sizes_rows = n;
    return NMN_OK;
}

// codes of n rows already on the device (stride ld) whose lists are assign_dev: PQ residual + encode, or Binary quantize -> host
nmn_status codec_encode(nmn_ivf* ivf, const float* rows_dev, uint32_t ld, const uint32_t* assign_dev, uint64_t n, uint8_t* out_host) {
    if (n == 0) return NMN_OK;
    hipStream_t s = ivf->stream;
    void* codes_dev = nullptr;
    float* res = nullptr;
    hipError_t e = hipMalloc(&codes_dev, std::max<size_t>((size_t)n * ivf->code_bytes, 64));
    if (ivf->kind == NMN_IVF_PQ) {
        if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&res), std::max<size_t>((size_t)n * ivf->dim * 4, 64));
        if (e == hipSuccess)
            e = launch_pq_residual(rows_dev, ld, ivf->centroids->corpus, ivf->centroids->ld, assign_dev, n, ivf->dim, ivf->pq_sub, res, s);
        if (e == hipSuccess)
            e = launch_pq_encode(res, n, ivf->pq_m, ivf->pq_sub, ivf->codebook, ivf->pq_k, static_cast<uint8_t*>(codes_dev), s);
    } else if (e == hipSuccess) {
        e = launch_bq_quantize(rows_dev, ld, n, ivf->dim, ivf->bq_method, static_cast<uint64_t*>(codes_dev), s);
    }
    if (e == hipSuccess) e = hipMemcpyAsync(out_host, codes_dev, (size_t)n * ivf->code_bytes, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (codes_dev) (void)hipFree(codes_dev);
    if (res) (void)hipFree(res);
    return e == hipSuccess ? NMN_OK : set_error_hip(e, "IVF encode");
}

}  // namespace

extern "C" void nmn_ivf_storage_default(nmn_ivf_storage* s) {  // IVFStorage::Flat, PQConfig::default (pq.rs:60-68), Sign
    if (!s) return;
    memset(s, 0, sizeof *s);
    s->kind = NMN_IVF_FLAT;
    s->pq_num_subspaces = 8;
    s->pq_num_centroids = 256;
    s->pq_kmeans.max_iterations = 100;  // KMeansConfig::default
    s->pq_kmeans.convergence_threshold = 1e-4f;
    s->pq_kmeans.seed = 42;
    s->pq_kmeans.init_method = 1;
    s->binary_threshold = NMN_BINARY_SIGN;
}

extern "C" nmn_status nmn_ivf_build_ex(const nmn_index_desc* desc, const float* rows_host, uint64_t n, uint32_t num_clusters,
                                       const nmn_kmeans_options* kmeans, const nmn_ivf_storage* storage, nmn_ivf** out) {
    if (!desc || !rows_host || !kmeans || !out) return set_error(NMN_ERR_INVALID_ARGUMENT, "null argument");
    *out = nullptr;
    if (!storage || storage->kind == NMN_IVF_FLAT) return ivf_train_flat(desc, rows_host, n, num_clusters, kmeans, true, out);
    nmn_status st = check_storage(storage, desc->dim);  // (the reference asserts in PQCodebook::train; no index is built here)
    if (st != NMN_OK) return st;
    if (n == 0 || num_clusters == 0) return set_error(NMN_ERR_INVALID_ARGUMENT, "nothing to train on");
    if (desc->capacity_rows < n) return set_error(NMN_ERR_CAPACITY, "capacity_rows < n");
    // IVFIndex::train's k-means and `find_nearest_centroid` of every vector: the Flat trainer over a transient copy of the rows
    nmn_index_desc td = *desc;
    td.capacity_rows = n;
    td.row_base = 0;
    nmn_ivf* t = nullptr;
    st = ivf_train_flat(&td, rows_host, n, num_clusters, kmeans, false, &t);
    if (st != NMN_OK) return st;
    struct Drop {
        nmn_ivf* p;
        ~Drop() {
            if (p) nmn_ivf_destroy(p);
        }
    } drop_t{t};
    const uint32_t C = t->n_clusters, dim = desc->dim;
    std::vector<float> codebook;
    uint32_t Kp = 0;
    if (storage->kind == NMN_IVF_PQ) {
        // PQCodebook::train (pq.rs:114-169) over the residuals: K' = min(num_centroids, n); subspace m = one KMeans::fit with
        // pq_config.kmeans_config over the m-th sub-vectors — the exact GPU k-means again, on an n x subdim index
        const uint32_t M = storage->pq_num_subspaces, sub = dim / M;
        Kp = (uint32_t)std::min<uint64_t>(storage->pq_num_centroids, n);
        codebook.assign((size_t)M * Kp * sub, 0.0f);  // (zero padding should a fit return fewer codewords, pq.rs:150-157)
        if (Kp) {
            float* res = nullptr;
            hipError_t e = hipSetDevice(t->device);
            if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&res), (size_t)n * dim * 4);
            if (e == hipSuccess)
                e = launch_pq_residual(t->vectors->corpus, t->vectors->ld, t->centroids->corpus, t->centroids->ld, t->assign, n, dim, sub, res,
                                       t->stream);
            std::vector<float> subv((size_t)n * sub);
            for (uint32_t m = 0; m < M && e == hipSuccess && st == NMN_OK; m++) {
                e = hipMemcpyAsync(subv.data(), res + (size_t)m * n * sub, subv.size() * 4, hipMemcpyDeviceToHost, t->stream);
                if (e == hipSuccess) e = hipStreamSynchronize(t->stream);
                if (e != hipSuccess) break;
                nmn_index_desc sd{};
                sd.dim = sub;
                sd.capacity_rows = n;
                sd.device = t->device;
                nmn_ivf* km = nullptr;
                st = ivf_train_flat(&sd, subv.data(), n, Kp, &storage->pq_kmeans, false, &km);
                if (st != NMN_OK) break;
                const size_t got = std::min(km->centroids_host.size(), (size_t)Kp * sub);
                std::copy(km->centroids_host.begin(), km->centroids_host.begin() + got, codebook.begin() + (size_t)m * Kp * sub);
                nmn_ivf_destroy(km);
            }
            if (res) (void)hipFree(res);
            if (e != hipSuccess) return set_error_hip(e, "IVF-PQ codebook training");
            if (st != NMN_OK) return st;
        }
    }
    nmn_ivf* ivf = nullptr;
    st = codec_new(desc, t->centroids_host.data(), C, storage, codebook.data(), Kp, &ivf);
    if (st != NMN_OK) return st;
    // `for vector in &vectors { index.add(vector) }`: the lists are the trainer's assignments, the codes come from its rows
    ivf->codes_host.resize((size_t)n * ivf->code_bytes);
    ivf->assign_host.assign(t->assign_host.begin(), t->assign_host.begin() + n);
    ivf->n_coded = n;
    st = codec_encode(ivf, t->vectors->corpus, t->vectors->ld, t->assign, n, ivf->codes_host.data());
    if (st == NMN_OK) st = codec_layout(ivf);
    if (st != NMN_OK) {
        nmn_ivf_destroy(ivf);
        return st;
    }
    *out = ivf;  // (the f32 rows go with `t` on return)
    return NMN_OK;
}

extern "C" nmn_status nmn_ivf_create_ex(const nmn_index_desc* desc, const float* centroids, uint32_t n_clusters,
                                        const nmn_ivf_storage* storage, const float* pq_codebook, uint32_t K, nmn_ivf** out) {
    if (!desc || !centroids || !out) return set_error(NMN_ERR_INVALID_ARGUMENT, "null argument");
    *out = nullptr;
    if (!storage || storage->kind == NMN_IVF_FLAT) return ivf_new(desc, centroids, n_clusters, out);
    nmn_status st = check_storage(storage, desc->dim);
    if (st != NMN_OK) return st;
    if (storage->kind == NMN_IVF_PQ && K && !pq_codebook) return set_error(NMN_ERR_INVALID_ARGUMENT, "null codebook");
    return codec_new(desc, centroids, n_clusters, storage, pq_codebook, storage->kind == NMN_IVF_PQ ? K : 0, out);
}

// IVFIndex::add (ivf.rs:276-316) for a PQ / Binary index: the rows pass through a transient flat index (padded like queries,
// so the exact centroid sweep scores them in place), get their lists and codes, and leave the device again
static nmn_status codec_add(nmn_ivf* ivf, const float* rows_host, uint64_t n, uint32_t* clusters_out) {
    if (ivf->n_coded + n > ivf->cap) return set_error(NMN_ERR_CAPACITY, "capacity_rows exceeded");
    IVF_TRY(hipSetDevice(ivf->device));
    const uint64_t row0 = ivf->n_coded;
    const uint64_t kStage = std::min<uint64_t>(n, 65536);
    nmn_index_desc sd{};
    sd.dim = ivf->dim;
    sd.flags = ivf->flags;
    sd.capacity_rows = kStage;
    sd.device = ivf->device;
    nmn_index* stg = nullptr;
    nmn_status st = nmn_index_create(&sd, &stg);
    if (st != NMN_OK) return st;
    uint32_t* assign_dev = nullptr;
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&assign_dev), kStage * 4);
    if (e != hipSuccess) {
        nmn_index_destroy(stg);
        return set_error_hip(e, "IVF add");
    }
    if (stg->ld != ivf->centroids->ld) st = set_error(NMN_ERR_STORAGE, "IVF add: staging layout differs from the centroids'");
    ivf->assign_host.resize(row0 + n);
    ivf->codes_host.resize((size_t)(row0 + n) * ivf->code_bytes);
    const uint32_t ld = stg->ld;
    for (uint64_t off = 0; off < n && st == NMN_OK; off += kStage) {
        const uint64_t cnt = std::min(kStage, n - off);
        st = nmn_index_upload(stg, rows_host + off * ivf->dim, 0, cnt);
        if (st != NMN_OK) break;
        e = hipStreamSynchronize(stg->host_stream);
        // find_nearest_centroid (ivf.rs:490-497): the same sweep + first minimum as Flat's add
        for (uint64_t a = 0; a < cnt && e == hipSuccess && st == NMN_OK; a += ivf->assign_chunk) {
            const uint32_t c = (uint32_t)std::min<uint64_t>(ivf->assign_chunk, cnt - a);
            st = centroid_scores(ivf, stg->corpus + a * ld, c);
            if (st != NMN_OK) break;
            hipLaunchKernelGGL(ivf_assign_kernel, dim3((c * 64 + 255) / 256), dim3(256), 0, ivf->stream, ivf->cscores, ivf->n_clusters, c, c,
                               assign_dev + a);
            e = hipGetLastError();
        }
        if (e == hipSuccess && st == NMN_OK)
            e = hipMemcpyAsync(ivf->assign_host.data() + row0 + off, assign_dev, cnt * 4, hipMemcpyDeviceToHost, ivf->stream);
        if (e == hipSuccess && st == NMN_OK)
            st = codec_encode(ivf, stg->corpus, ld, assign_dev, cnt, ivf->codes_host.data() + (size_t)(row0 + off) * ivf->code_bytes);
        if (e != hipSuccess && st == NMN_OK) st = set_error_hip(e, "IVF add");
    }
    (void)hipFree(assign_dev);
    nmn_index_destroy(stg);
    if (st != NMN_OK) {
        ivf->assign_host.resize(row0);
        ivf->codes_host.resize((size_t)row0 * ivf->code_bytes);
        return st;
    }
    if (clusters_out) memcpy(clusters_out, ivf->assign_host.data() + row0, n * 4);
    ivf->n_coded = row0 + n;
    return codec_layout(ivf);
}

static nmn_status codec_search(nmn_ivf* ivf, const float* queries, uint32_t nq, uint32_t k, uint32_t nprobe, uint64_t* out_ids,
                               float* out_distances, uint32_t* out_counts) {
    for (uint32_t q = 0; q < nq; q++) {  // unused slots as Flat's: id UINT64_MAX, distance +inf
        std::fill(out_ids + (size_t)q * k, out_ids + (size_t)(q + 1) * k, UINT64_MAX);
        std::fill(out_distances + (size_t)q * k, out_distances + (size_t)(q + 1) * k, __builtin_inff());
        out_counts[q] = 0;
    }
    const uint32_t C = ivf->n_clusters, dim = ivf->dim;
    const uint32_t np = std::min<uint32_t>(nprobe, C);  // ivf.rs:339
    if (ivf->n_coded == 0 || np == 0) return NMN_OK;
    std::lock_guard<std::mutex> lk(ivf->codec_mu);
    IVF_TRY(hipSetDevice(ivf->device));
    hipStream_t s = ivf->stream;
    const uint32_t ld = ivf->centroids->ld;
    const uint32_t chunk = C <= kRankMax ? std::min<uint32_t>(nq, 64) : 1u;
    nmn_ivf::CodecScratch& cs = ivf->cs;
    bool wait = false;  // (every coded search ends with a wait of its own: nothing enqueued still reads the scratch)
    auto need = [&](Grow& g, size_t bytes) { return g.reserve(bytes, s, wait); };
    IVF_TRY(cs.rank.reserve(ivf, chunk, true, s, wait));
    std::vector<uint64_t> probe_host((size_t)C * chunk);
    std::vector<uint32_t> pcount(chunk);
    const size_t seg_bytes = codec_seg_bytes();
    struct Seg {
        uint32_t list, start, count, cand;
    };
    static_assert(sizeof(Seg) == 16, "CodecSeg layout");
    if (seg_bytes != sizeof(Seg)) return set_error(NMN_ERR_STORAGE, "IVF codec: segment layout mismatch");
    constexpr uint64_t kScoreBudget = 64ull << 20;  // candidates' scores per scan launch (256 MiB)
    const uint32_t Kt = std::min<uint32_t>(ivf->pq_k, 256);
    for (uint32_t q0 = 0; q0 < nq; q0 += chunk) {
        const uint32_t nb = std::min<uint32_t>(chunk, nq - q0);
        // 1. the centroid ranking of the chunk, exactly as Flat ranks (squared distance ascending, ties by index)
        IVF_TRY(hipMemcpyAsync(cs.rank.qraw.p, queries + (size_t)q0 * dim, (size_t)nb * dim * 4, hipMemcpyHostToDevice, s));
        nmn_status st = rank_centroids(ivf, gp<float>(cs.rank.qraw), nb, np, cs.rank, false, s);
        if (st != NMN_OK) return st;
        if (C <= kRankMax) {
            IVF_TRY(hipMemcpyAsync(probe_host.data(), cs.rank.probe_rows.p, (size_t)nb * C * 8, hipMemcpyDeviceToHost, s));
        } else {
            IVF_TRY(hipMemcpyAsync(probe_host.data(), cs.rank.probe_rows.p, (size_t)np * 8, hipMemcpyDeviceToHost, s));
        }
        IVF_TRY(hipMemcpyAsync(pcount.data(), cs.rank.probe_count.p, (size_t)nb * 4, hipMemcpyDeviceToHost, s));
        IVF_TRY(hipStreamSynchronize(s));
        // 2. candidates = the probed lists in probe order, each in list order (= id order)
        const size_t pstride = C <= kRankMax ? C : 0;
        std::vector<Seg> segs((size_t)nb * np);
        std::vector<uint64_t> total(nb, 0);
        uint32_t max_count = 0;
        for (uint32_t b = 0; b < nb; b++) {
            const uint32_t cnt = std::min(pcount[b], np);
            uint64_t cand = 0;
            for (uint32_t i = 0; i < np; i++) {
                Seg& sg = segs[(size_t)b * np + i];
                sg = Seg{0, 0, 0, (uint32_t)cand};
                const uint64_t c = probe_host[(size_t)b * pstride + i];
                if (i >= cnt || c >= C) continue;
                sg.list = (uint32_t)c;
                sg.start = ivf->list_off_host[c];
                sg.count = ivf->list_off_host[c + 1] - ivf->list_off_host[c];
                cand += sg.count;
                max_count = std::max(max_count, sg.count);
            }
            total[b] = cand;
        }
        // 3. scans + one large-k sort per query, in groups whose scores fit the budget
        for (uint32_t g0 = 0; g0 < nb;) {
            uint32_t g1 = g0 + 1;
            uint64_t sum = total[g0];
            while (g1 < nb && sum + total[g1] <= kScoreBudget) sum += total[g1++];
            const uint32_t ng = g1 - g0;
            std::vector<uint64_t> base(ng), rbase(ng);
            uint64_t max_total = 0, rsum = 0;
            for (uint32_t b = 0; b < ng; b++) {
                base[b] = b ? base[b - 1] + total[g0 + b - 1] : 0;
                rbase[b] = rsum;
                rsum += std::min<uint64_t>(k, total[g0 + b]);
                max_total = std::max(max_total, total[g0 + b]);
            }
            IVF_TRY(need(cs.segs, (size_t)ng * np * sizeof(Seg)));
            IVF_TRY(need(cs.base, (size_t)ng * 8));
            IVF_TRY(need(cs.scores, (size_t)sum * 4));
            IVF_TRY(need(cs.keys, largek_sort_len(std::max<uint64_t>(max_total, 1)) * 8));
            IVF_TRY(need(cs.rows, (size_t)rsum * 8));
            IVF_TRY(need(cs.rscores, (size_t)rsum * 4));
            IVF_TRY(need(cs.rcnt, (size_t)ng * 4));
            IVF_TRY(hipMemcpyAsync(cs.segs.p, segs.data() + (size_t)g0 * np, (size_t)ng * np * sizeof(Seg), hipMemcpyHostToDevice, s));
            IVF_TRY(hipMemcpyAsync(cs.base.p, base.data(), (size_t)ng * 8, hipMemcpyHostToDevice, s));
            const float* qg = gp<float>(cs.rank.qraw) + (size_t)g0 * dim;
            if (ivf->kind == NMN_IVF_PQ) {
                IVF_TRY(need(cs.tables, (size_t)ng * np * ivf->pq_m * Kt * 4));
                IVF_TRY(launch_pq_search(qg, dim, ivf->centroids->corpus, ld, cs.segs.p, np, ng, max_count, ivf->codebook, ivf->pq_k,
                                         ivf->pq_m, ivf->lcodes, gp<float>(cs.tables), gp<uint64_t>(cs.base),
                                         gp<uint32_t>(cs.scores), s));
            } else {
                const uint32_t W = (dim + 63) / 64;
                IVF_TRY(need(cs.qwords, (size_t)ng * W * 8));
                IVF_TRY(launch_bq_quantize(qg, dim, ng, dim, ivf->bq_method, gp<uint64_t>(cs.qwords), s));
                IVF_TRY(launch_bq_search(gp<uint64_t>(cs.qwords), dim, cs.segs.p, np, ng, max_count,
                                         reinterpret_cast<const uint64_t*>(ivf->lcodes), gp<uint64_t>(cs.base),
                                         gp<uint32_t>(cs.scores), s));
            }
            IVF_TRY(hipMemsetAsync(cs.rcnt.p, 0, (size_t)ng * 4, s));
            for (uint32_t b = 0; b < ng; b++) {
                const uint64_t tot = total[g0 + b];
                if (tot == 0) continue;
                const uint32_t kq = (uint32_t)std::min<uint64_t>(k, tot);
                IVF_TRY(launch_largek(gp<uint32_t>(cs.scores) + base[b], tot, gp<uint64_t>(cs.keys), kq, 0,
                                      gp<uint64_t>(cs.rows) + rbase[b], gp<float>(cs.rscores) + rbase[b],
                                      gp<uint32_t>(cs.rcnt) + b, s));
            }
            std::vector<uint64_t> rrows(rsum);
            std::vector<float> rsc(rsum);
            std::vector<uint32_t> rcnt(ng);
            if (rsum) {
                IVF_TRY(hipMemcpyAsync(rrows.data(), cs.rows.p, rsum * 8, hipMemcpyDeviceToHost, s));
                IVF_TRY(hipMemcpyAsync(rsc.data(), cs.rscores.p, rsum * 4, hipMemcpyDeviceToHost, s));
            }
            IVF_TRY(hipMemcpyAsync(rcnt.data(), cs.rcnt.p, (size_t)ng * 4, hipMemcpyDeviceToHost, s));
            IVF_TRY(hipStreamSynchronize(s));
            // 4. candidate index -> (probed list, position) -> id; distance = -score
            for (uint32_t b = 0; b < ng; b++) {
                const uint32_t q = q0 + g0 + b;
                const Seg* sq = segs.data() + (size_t)(g0 + b) * np;
                const uint32_t cnt = std::min<uint32_t>(rcnt[b], (uint32_t)std::min<uint64_t>(k, total[g0 + b]));
                for (uint32_t j = 0; j < cnt; j++) {
                    const uint64_t cand = rrows[rbase[b] + j];
                    uint32_t lo = 0, hi = np;  // last segment whose first candidate <= cand (empty ones share offsets: take the last)
                    while (hi - lo > 1) {
                        const uint32_t mid = (lo + hi) >> 1;
                        if (sq[mid].cand <= cand) lo = mid;
                        else hi = mid;
                    }
                    while (sq[lo].count == 0 || cand - sq[lo].cand >= sq[lo].count) lo--;  // (never below 0: cand < total)
                    out_ids[(size_t)q * k + j] = ivf->row_base + ivf->perm_host[sq[lo].start + (cand - sq[lo].cand)];
                    out_distances[(size_t)q * k + j] = 0.0f - rsc[rbase[b] + j];
                }
                out_counts[q] = cnt;
            }
            g0 = g1;
        }
    }
    return NMN_OK;
}

// ---- nmn_ivf_search_device: the whole search in stream order (docs/ivf.md §3.10c) ----------------------------------------------
// One pipeline for every storage, nothing read back: centroid ranking (as above) -> ivf_plan_kernel (the probed lists of each
// query as segments of its candidates, from the device list offsets) -> a scan writing the negated distance of every candidate
// in candidate order (Flat: launch_ivf_flat_scan, exact f32; PQ / Binary: the codec scans) -> ivf_select_kernel (k <= 4096: the
// k best by (score desc, candidate asc) = the reference's stable sort, one workgroup per query) or the large-k sort -> ivf_idmap_kernel
// (candidate -> list-major row -> id, distance = -score).  Per query the scores take a slot of `bound` = the rows of the np
// largest lists, which the host knows, so every grid and buffer is sized without looking at the probe orders.
namespace {

constexpr uint32_t kSelMax = 4096;  // ivf_select_kernel's LDS list

// query blockIdx.x: segs[q * np + i] = {list, first row, rows, first candidate} of its i-th probed list (empty past the probe
// count), totals[q] = its candidates, base[q] = q * stride (where its scores start)
__global__ __launch_bounds__(64) void ivf_plan_kernel(const uint64_t* __restrict__ probe_rows, uint32_t pstride,
                                                      const uint32_t* __restrict__ probe_count, uint32_t np, uint32_t n_clusters,
                                                      const uint32_t* __restrict__ off, uint64_t stride, uint4* __restrict__ segs,
                                                      uint64_t* __restrict__ totals, uint64_t* __restrict__ base) {
    const uint32_t q = blockIdx.x, lane = threadIdx.x;
    const uint32_t cnt = min(probe_count[q], np);
    uint32_t run = 0;
    for (uint32_t i0 = 0; i0 < np; i0 += 64) {
        const uint32_t i = i0 + lane;
        uint32_t list = 0, start = 0, count = 0;
        if (i < cnt) {
            const uint64_t c = probe_rows[(size_t)q * pstride + i];
            if (c < n_clusters) {
                list = (uint32_t)c;
                start = off[c];
                count = off[c + 1] - start;
            }
        }
        uint32_t x = count;  // inclusive prefix over the wave = candidates up to and including probe i
        for (uint32_t o = 1; o < 64; o <<= 1) {
            const uint32_t y = __shfl_up(x, o);
            if (lane >= o) x += y;
        }
        if (i < np) segs[(size_t)q * np + i] = make_uint4(list, start, count, run + x - count);
        run += __shfl(x, 63);
    }
    if (lane == 0) {
        totals[q] = run;
        base[q] = (uint64_t)q * stride;
    }
}

// the k best candidates of query blockIdx.x (k <= kSelMax): composite keys (score key << 32 | ~candidate) — descending composite
// = score descending, candidate ascending.  A radix select (8 bits a pass, histograms in LDS) finds the key T of the k-th; every
// key above T and the first (in candidate order) of those equal to it go to LDS, a bitonic sort orders them.  Writes the
// candidate index and the score; ivf_idmap_kernel turns them into ids and distances.
__global__ __launch_bounds__(1024) void ivf_select_kernel(const uint32_t* __restrict__ scores, uint64_t stride,
                                                          const uint64_t* __restrict__ totals, uint32_t k, uint64_t* __restrict__ out_cand,
                                                          float* __restrict__ out_score) {
    __shared__ uint64_t sel[kSelMax];
    __shared__ uint32_t hist[256];
    __shared__ uint32_t wsum[16];
    __shared__ uint32_t sh[4];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6, q = blockIdx.x;
    const uint64_t total = totals[q];
    const uint32_t need = (uint32_t)min<uint64_t>(k, total);
    if (need == 0) return;
    const uint32_t* sc = scores + (uint64_t)q * stride;
    auto composite = [](uint32_t key, uint64_t i) { return ((uint64_t)key << 32) | (uint32_t)~(uint32_t)i; };
    uint32_t n_sort = need;
    if (total <= kSelMax) {  // everything fits: sort it all
        n_sort = (uint32_t)total;
        for (uint32_t i = tid; i < n_sort; i += 1024) sel[i] = composite(bits_to_key(sc[i]), i);
    } else {
        uint32_t prefix = 0, pmask = 0, r = need - 1;  // r: descending rank of the k-th among the keys matching prefix
        for (int shift = 24; shift >= 0; shift -= 8) {
            for (uint32_t b = tid; b < 256; b += 1024) hist[b] = 0;
            __syncthreads();
            for (uint64_t i = tid; i < total; i += 1024) {
                const uint32_t key = bits_to_key(sc[i]);
                if ((key & pmask) == prefix) atomicAdd(&hist[(key >> shift) & 0xFFu], 1u);
            }
            __syncthreads();
            if (tid == 0) {
                uint32_t b = 255, above = 0;
                while (above + hist[b] <= r) above += hist[b--];
                sh[0] = b;
                sh[1] = r - above;
            }
            __syncthreads();
            prefix |= sh[0] << shift;
            pmask |= 0xFFu << shift;
            r = sh[1];
            __syncthreads();
        }
        const uint32_t T = prefix, take_eq = r + 1, n_gt = need - take_eq;
        if (tid == 0) {
            sh[2] = 0;  // keys above T placed
            sh[3] = 0;  // keys equal to T seen, in candidate order
        }
        __syncthreads();
        for (uint64_t i0 = 0; i0 < total; i0 += 1024) {
            const uint64_t i = i0 + tid;
            const uint32_t key = i < total ? bits_to_key(sc[i]) : 0u;
            if (key > T) sel[atomicAdd(&sh[2], 1u)] = composite(key, i);  // (exactly n_gt of them in all)
            const bool eq = i < total && key == T;
            const uint64_t bal = __ballot(eq);
            if (lane == 0) wsum[wave] = (uint32_t)__popcll(bal);
            __syncthreads();
            uint32_t before = sh[3];
            for (uint32_t w = 0; w < wave; w++) before += wsum[w];
            if (eq) {
                const uint32_t rank = before + (uint32_t)__popcll(bal & ((1ull << lane) - 1ull));
                if (rank < take_eq) sel[n_gt + rank] = composite(key, i);
            }
            __syncthreads();
            if (tid == 0) {
                uint32_t t = 0;
                for (uint32_t w = 0; w < 16; w++) t += wsum[w];
                sh[3] += t;
            }
            __syncthreads();
        }
    }
    uint32_t np2 = 1;
    while (np2 < n_sort) np2 <<= 1;
    for (uint32_t i = n_sort + tid; i < np2; i += 1024) sel[i] = 0;  // (sorts last)
    __syncthreads();
    for (uint32_t size = 2; size <= np2; size <<= 1) {
        for (uint32_t stride2 = size >> 1; stride2 > 0; stride2 >>= 1) {
            for (uint32_t p = tid; p < (np2 >> 1); p += 1024) {
                const uint32_t lo = ((p & ~(stride2 - 1)) << 1) | (p & (stride2 - 1));
                const uint32_t hi = lo + stride2;
                const bool desc = (lo & size) == 0;
                const uint64_t a = sel[lo], b = sel[hi];
                if ((a < b) == desc) {
                    sel[lo] = b;
                    sel[hi] = a;
                }
            }
            __syncthreads();
        }
    }
    out_cand += (size_t)q * k;
    out_score += (size_t)q * k;
    for (uint32_t i = tid; i < need; i += 1024) {
        out_cand[i] = (uint32_t)~(uint32_t)sel[i];
        out_score[i] = key_to_score((uint32_t)(sel[i] >> 32));
    }
}

// candidates [totals[q], stride) of query blockIdx.y take no part in the large-k sort
__global__ __launch_bounds__(256) void ivf_pad_kernel(uint32_t* __restrict__ scores, uint64_t stride, const uint64_t* __restrict__ totals) {
    const uint32_t q = blockIdx.y;
    for (uint64_t i = totals[q] + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < stride; i += (uint64_t)gridDim.x * blockDim.x)
        scores[(uint64_t)q * stride + i] = kScoreSentinelBits;
}

// slots [0, k) of query blockIdx.y: candidate j (as selected) -> its segment (the last one starting at or before j that holds
// rows) -> list-major row -> id; distance = 0 - score (as the host call and codec_search form it); the rest id UINT64_MAX, distance +inf.  totals == nullptr: nothing found (empty index, nprobe 0).
__global__ __launch_bounds__(256) void ivf_idmap_kernel(const uint4* __restrict__ segs, uint32_t np, const uint64_t* __restrict__ totals,
                                                        const uint32_t* __restrict__ perm, uint64_t id_base, int flat, uint32_t k,
                                                        uint64_t* __restrict__ ids, float* __restrict__ dist, uint32_t* __restrict__ counts) {
    (void)flat;
    const uint32_t q = blockIdx.y;
    const uint32_t cnt = totals ? (uint32_t)min<uint64_t>(k, totals[q]) : 0u;
    ids += (size_t)q * k;
    dist += (size_t)q * k;
    const uint4* sq = segs ? segs + (size_t)q * np : nullptr;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < k; i += gridDim.x * blockDim.x) {
        if (i < cnt) {
            const uint32_t cand = (uint32_t)ids[i];
            const float s = dist[i];
            uint32_t lo = 0, hi = np;
            while (hi - lo > 1) {
                const uint32_t mid = (lo + hi) >> 1;
                if (sq[mid].w <= cand) lo = mid;
                else hi = mid;
            }
            while (sq[lo].z == 0 || cand - sq[lo].w >= sq[lo].z) lo--;  // (never below 0: cand < total)
            ids[i] = id_base + perm[sq[lo].y + (cand - sq[lo].w)];
            dist[i] = 0.0f - s;  // (a zero distance comes back as +0.0 whatever the sign of the zero score, as the host call's)
        } else {
            ids[i] = UINT64_MAX;
            dist[i] = __builtin_inff();
        }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) counts[q] = cnt;
}

// the candidate-order id map and list offsets of the current index state on the device (caller holds rw shared and dev_mu)
nmn_status dev_map_build(nmn_ivf* ivf, hipStream_t s) {
    const bool flat = ivf->kind == NMN_IVF_FLAT;
    const uint64_t n = flat ? ivf->vectors->rows : ivf->n_coded;
    const uint32_t C = ivf->n_clusters;
    std::vector<uint32_t> off((size_t)C + 1, 0u), perm_flat;
    const uint32_t* perm = ivf->perm_host.data();
    if (flat) {  // every vector by list, ids ascending inside a list: list-major rows, then the younger ones of the same list
        if (ivf->assign_host.size() < n) return set_error(NMN_ERR_STORAGE, "IVF lists are not current");
        for (uint64_t r = 0; r < n; r++) off[ivf->assign_host[r] + 1]++;
        for (uint32_t c = 0; c < C; c++) off[c + 1] += off[c];
        perm_flat.resize(n);
        std::vector<uint32_t> cur(off.begin(), off.end() - 1);
        for (uint64_t r = 0; r < n; r++) perm_flat[cur[ivf->assign_host[r]]++] = (uint32_t)r;
        perm = perm_flat.data();
    } else {  // the list-major codes' own layout (codec_layout)
        if (ivf->list_off_host.size() != (size_t)C + 1 || ivf->perm_host.size() < n) return set_error(NMN_ERR_STORAGE, "IVF lists are not current");
        off.assign(ivf->list_off_host.begin(), ivf->list_off_host.end());
    }
    // (the searches that read the previous map have finished: `add` waited for them before it changed the index)
    if (ivf->dev_perm) (void)hipFree(ivf->dev_perm);
    if (ivf->dev_off) (void)hipFree(ivf->dev_off);
    ivf->dev_perm = nullptr;
    ivf->dev_off = nullptr;
    ivf->dev_gen = ~0ull;
    IVF_TRY(hipMalloc(reinterpret_cast<void**>(&ivf->dev_perm), std::max<uint64_t>(n, 1) * 4));
    IVF_TRY(hipMalloc(reinterpret_cast<void**>(&ivf->dev_off), ((size_t)C + 1) * 4));
    if (n) IVF_TRY(hipMemcpyAsync(ivf->dev_perm, perm, n * 4, hipMemcpyHostToDevice, s));
    IVF_TRY(hipMemcpyAsync(ivf->dev_off, off.data(), ((size_t)C + 1) * 4, hipMemcpyHostToDevice, s));
    IVF_TRY(hipStreamSynchronize(s));  // (the host arrays go out of scope)
    std::vector<uint64_t> sizes(C);
    for (uint32_t c = 0; c < C; c++) sizes[c] = off[c + 1] - off[c];
    std::sort(sizes.begin(), sizes.end(), std::greater<uint64_t>());
    ivf->dev_top.assign((size_t)C + 1, 0);
    for (uint32_t c = 0; c < C; c++) ivf->dev_top[c + 1] = ivf->dev_top[c] + sizes[c];
    ivf->dev_rows = n;
    ivf->dev_gen = ivf->gen;
    return NMN_OK;
}

}  // namespace

extern "C" nmn_status nmn_ivf_search_device(nmn_ivf* ivf, const float* queries_dev, uint32_t nq, uint32_t k, uint32_t nprobe,
                                            uint64_t* out_ids_dev, float* out_distances_dev, uint32_t* out_counts_dev, void* stream) {
    if (!ivf || !queries_dev || !out_ids_dev || !out_distances_dev || !out_counts_dev)
        return set_error(NMN_ERR_INVALID_ARGUMENT, "null argument");
    if (k == 0) return set_error(NMN_ERR_INVALID_TOP_K, "k == 0");
    if (nq == 0) return NMN_OK;
    std::shared_lock<std::shared_mutex> g(ivf->rw);  // concurrent with other searches, not with add / build
    IVF_TRY(hipSetDevice(ivf->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    const bool flat = ivf->kind == NMN_IVF_FLAT;
    const uint64_t n = flat ? ivf->vectors->rows : ivf->n_coded;
    const uint32_t C = ivf->n_clusters, dim = ivf->dim;
    const uint32_t np = std::min<uint32_t>(nprobe, C);  // ivf.rs:339
    const bool empty = n == 0 || np == 0;
    nmn_ivf::DevScratch* sc = nullptr;
    const uint32_t* perm = nullptr;
    const uint32_t* off = nullptr;
    uint64_t bound = 0, max_list = 0;
    {
        std::lock_guard<std::mutex> lk(ivf->dev_mu);
        if (!empty && ivf->dev_gen != ivf->gen) {
            nmn_status st = dev_map_build(ivf, s);
            if (st != NMN_OK) return st;
        }
        for (auto& x : ivf->dev_scratch)
            if (x->stream == s) sc = x.get();
        if (!sc) {
            ivf->dev_scratch.push_back(std::make_unique<nmn_ivf::DevScratch>());
            sc = ivf->dev_scratch.back().get();
            sc->stream = s;
        }
        perm = ivf->dev_perm;
        off = ivf->dev_off;
        if (!empty) {
            bound = std::max<uint64_t>(ivf->dev_top[np], 1);
            max_list = ivf->dev_top[1];
        }
    }
    std::lock_guard<std::mutex> slk(sc->mu);
    const uint64_t id_base = flat ? ivf->vectors->row_base : ivf->row_base;
    auto record = [&]() -> nmn_status {  // the event add / destroy wait for
        std::lock_guard<std::mutex> lk(ivf->dev_mu);
        for (size_t i = 0; i < ivf->ev_pending.size();) {  // recycle the completed ones (a query, not a wait)
            if (hipEventQuery(ivf->ev_pending[i]) == hipSuccess) {
                ivf->ev_free.push_back(ivf->ev_pending[i]);
                ivf->ev_pending[i] = ivf->ev_pending.back();
                ivf->ev_pending.pop_back();
            } else {
                i++;
            }
        }
        hipEvent_t e = nullptr;
        if (!ivf->ev_free.empty()) {
            e = ivf->ev_free.back();
            ivf->ev_free.pop_back();
        } else {
            IVF_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        }
        const hipError_t he = hipEventRecord(e, s);
        if (he != hipSuccess) {
            ivf->ev_free.push_back(e);
            return set_error_hip(he, "nmn_ivf_search_device");
        }
        ivf->ev_pending.push_back(e);
        return NMN_OK;
    };
    if (empty) {  // unused slots and zero counts, on the stream
        hipLaunchKernelGGL(ivf_idmap_kernel, dim3((uint32_t)std::min<uint64_t>(((uint64_t)k + 255) / 256, 4096), nq), dim3(256), 0, s, nullptr, 0u,
                           nullptr, nullptr, 0ull, 0, k, out_ids_dev, out_distances_dev, out_counts_dev);
        IVF_TRY(hipGetLastError());
        return record();
    }
    if (codec_seg_bytes() != sizeof(uint4)) return set_error(NMN_ERR_STORAGE, "IVF: segment layout mismatch");
    const uint32_t ld = ivf->centroids->ld;
    const bool big_c = C > kRankMax;  // (the large-k sort ranks the centroids, one query at a time)
    constexpr uint64_t kScoreBudget = 64ull << 20;  // candidates' scores per chunk (256 MiB)
    uint32_t chunk = big_c ? 1u : std::min<uint32_t>(nq, 64);
    chunk = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(chunk, kScoreBudget / bound));
    const uint32_t Kt = std::min<uint32_t>(ivf->pq_k, 256), W = (dim + 63) / 64;
    // grow-only scratch of this stream's device searches: a buffer that must grow waits for the stream first (the calls before this
    // one may still read it) — the only wait of the pipeline, at most one per call, never in steady state
    bool wait = true;
    hipError_t ge = sc->rank.reserve(ivf, chunk, false, s, wait);
    auto need = [&](Grow& g, size_t bytes) {
        if (ge == hipSuccess) ge = g.reserve(bytes, s, wait);
    };
    need(sc->segs, (size_t)chunk * np * sizeof(uint4));
    need(sc->base, (size_t)chunk * 8);
    need(sc->totals, (size_t)chunk * 8);
    need(sc->scores, (size_t)chunk * bound * 4);
    if (k > kSelMax) need(sc->keys, largek_sort_len(bound) * 8);
    if (ivf->kind == NMN_IVF_PQ) need(sc->tables, (size_t)chunk * np * ivf->pq_m * Kt * 4);
    if (ivf->kind == NMN_IVF_BINARY) need(sc->qwords, (size_t)chunk * W * 8);
    if (ge != hipSuccess) return set_error_hip(ge, "nmn_ivf_search_device (scratch)");
    auto* segs = gp<uint4>(sc->segs);
    for (uint32_t q0 = 0; q0 < nq; q0 += chunk) {
        const uint32_t nb = std::min<uint32_t>(chunk, nq - q0);
        const float* qg = queries_dev + (size_t)q0 * dim;
        uint64_t* o_ids = out_ids_dev + (size_t)q0 * k;
        float* o_dist = out_distances_dev + (size_t)q0 * k;
        uint32_t* o_cnt = out_counts_dev + q0;
        // 1. centroid ranking, the host call's
        nmn_status st = rank_centroids(ivf, qg, nb, np, sc->rank, false, s);
        if (st != NMN_OK) return st;
        // 2. candidate plan
        hipLaunchKernelGGL(ivf_plan_kernel, dim3(nb), dim3(64), 0, s, gp<uint64_t>(sc->rank.probe_rows), C, gp<uint32_t>(sc->rank.probe_count), np, C,
                           off, bound, segs, gp<uint64_t>(sc->totals), gp<uint64_t>(sc->base));
        IVF_TRY(hipGetLastError());
        // 3. scores of every candidate, in candidate order
        if (flat) {
            IVF_TRY(launch_ivf_flat_scan(qg, dim, ivf->vectors->corpus, ivf->vectors->ld, perm, segs, np, nb, (uint32_t)max_list,
                                         gp<uint64_t>(sc->base), gp<uint32_t>(sc->scores), s));
        } else if (ivf->kind == NMN_IVF_PQ) {
            IVF_TRY(launch_pq_search(qg, dim, ivf->centroids->corpus, ld, segs, np, nb, (uint32_t)max_list, ivf->codebook, ivf->pq_k,
                                     ivf->pq_m, ivf->lcodes, gp<float>(sc->tables), gp<uint64_t>(sc->base), gp<uint32_t>(sc->scores), s));
        } else {
            IVF_TRY(launch_bq_quantize(qg, dim, nb, dim, ivf->bq_method, gp<uint64_t>(sc->qwords), s));
            IVF_TRY(launch_bq_search(gp<uint64_t>(sc->qwords), dim, segs, np, nb, (uint32_t)max_list,
                                     reinterpret_cast<const uint64_t*>(ivf->lcodes), gp<uint64_t>(sc->base), gp<uint32_t>(sc->scores), s));
        }
        // 4. selection: (score desc, candidate asc)
        if (k <= kSelMax) {
            hipLaunchKernelGGL(ivf_select_kernel, dim3(nb), dim3(1024), 0, s, gp<uint32_t>(sc->scores), bound, gp<uint64_t>(sc->totals), k,
                               o_ids, o_dist);
            IVF_TRY(hipGetLastError());
        } else {
            const uint32_t pad_blocks = (uint32_t)std::min<uint64_t>((bound + 255) / 256, 1024);
            hipLaunchKernelGGL(ivf_pad_kernel, dim3(pad_blocks, nb), dim3(256), 0, s, gp<uint32_t>(sc->scores), bound, gp<uint64_t>(sc->totals));
            IVF_TRY(hipGetLastError());
            for (uint32_t b = 0; b < nb; b++)
                IVF_TRY(launch_largek(gp<uint32_t>(sc->scores) + (size_t)b * bound, bound, gp<uint64_t>(sc->keys), k, 0, o_ids + (size_t)b * k,
                                      o_dist + (size_t)b * k, o_cnt + b, s));
        }
        // 5. ids, distances, counts
        hipLaunchKernelGGL(ivf_idmap_kernel, dim3((uint32_t)std::min<uint64_t>(((uint64_t)k + 255) / 256, 4096), nb), dim3(256), 0, s, segs, np,
                           gp<uint64_t>(sc->totals), perm, id_base, flat ? 1 : 0, k, o_ids, o_dist, o_cnt);
        IVF_TRY(hipGetLastError());
    }
    return record();
}

extern "C" int32_t nmn_ivf_storage_kind(const nmn_ivf* ivf) { return ivf ? ivf->kind : NMN_IVF_FLAT; }
extern "C" uint32_t nmn_ivf_pq_codewords(const nmn_ivf* ivf) { return (ivf && ivf->kind == NMN_IVF_PQ) ? ivf->pq_k : 0; }

extern "C" nmn_status nmn_ivf_pq_codebook(nmn_ivf* ivf, float* out, uint64_t cap_floats) {
    if (!ivf || !out) return set_error(NMN_ERR_INVALID_ARGUMENT, "null argument");
    if (ivf->kind != NMN_IVF_PQ) return set_error(NMN_ERR_CONFIGURATION, "not an IVF-PQ index");
    std::shared_lock<std::shared_mutex> g(ivf->rw);
    if (cap_floats < ivf->codebook_host.size()) return set_error(NMN_ERR_BUFFER_TOO_SMALL, "codebook buffer too small");
    std::copy(ivf->codebook_host.begin(), ivf->codebook_host.end(), out);
    return NMN_OK;
}

extern "C" nmn_status nmn_ivf_codes(nmn_ivf* ivf, void* out, uint64_t cap_bytes) {
    if (!ivf || !out) return set_error(NMN_ERR_INVALID_ARGUMENT, "null argument");
    if (ivf->kind == NMN_IVF_FLAT) return set_error(NMN_ERR_CONFIGURATION, "an IVF-Flat index holds no codes");
    std::shared_lock<std::shared_mutex> g(ivf->rw);
    const size_t need = (size_t)ivf->n_coded * ivf->code_bytes;
    if (cap_bytes < need) return set_error(NMN_ERR_BUFFER_TOO_SMALL, "code buffer too small");
    if (need) memcpy(out, ivf->codes_host.data(), need);
    return NMN_OK;
}

extern "C" uint64_t nmn_ivf_hbm_bytes(nmn_ivf* ivf) {
    if (!ivf) return 0;
    std::unique_lock<std::shared_mutex> g(ivf->rw);
    uint64_t b = index_hbm_bytes(ivf->vectors) + index_hbm_bytes(ivf->cvec) + index_hbm_bytes(ivf->centroids);
    if (ivf->kind == NMN_IVF_FLAT)  // the list of every row; the list-major copy's offsets
        b += std::max<uint64_t>(ivf->cap, 1) * 4 + (ivf->list_off ? ((uint64_t)ivf->n_clusters + 1) * 4 : 0);
    else  // the codes, the codebook (and the 64 bytes `assign` is without rows of its own)
        b += std::max<uint64_t>(ivf->cap, 1) * ivf->code_bytes + ivf->codebook_host.size() * 4 + 64;
    b += ivf->cscores_cap * 4 + sizeof(QInfo) * kAssignChunk;  // the assignment sweep's scores and its zero query records
    // the search scratch: what nmn_ivf_destroy frees, through the same enumerators
    auto count = [&](const Grow& g) {
        if (!g.pinned) b += g.cap;
    };
    for (auto& sl : ivf->slots) sl->for_each(count);
    ivf->cs.for_each(count);
    {   // what device searches added: the candidate-order id map and the per-stream scratch (nothing before the first one)
        std::lock_guard<std::mutex> lk(ivf->dev_mu);
        if (ivf->dev_perm) b += std::max<uint64_t>(ivf->dev_rows, 1) * 4 + ((uint64_t)ivf->n_clusters + 1) * 4;
        for (auto& sc : ivf->dev_scratch) sc->for_each(count);
    }
    return b;
}

// ---- persistence of the device layout ------------------------------------------------------------------
// File = Header{kind = ivf, dim, rows = vectors, aux = clusters} | centroids clusters x dim f32 | assign[] rows x u32 | a flat
// shard section (nmn_persist.hip) holding the vectors in id order.  A load re-creates the index WITHOUT re-running k-means or
// the list assignment: centroids and lists come back exactly as saved (the reference rebuilds its IVF index from the
// vectors after a restart; the trained centroids are the expensive part — tensor_store/src/ivf.rs:222-233).
#include "nmn_persist.h"

namespace nmn {
nmn_status persist_write_ivf(nmn_ivf* ivf, FILE* fp, const char* path) {
    if (ivf->kind != NMN_IVF_FLAT)
        return set_error(NMN_ERR_CONFIGURATION, "IVF-PQ / IVF-Binary indexes cannot be saved (only IVF-Flat persists its device layout)");
    std::unique_lock<std::shared_mutex> g(ivf->rw);
    const uint64_t rows = ivf->vectors->rows;
    std::vector<float> cents((size_t)ivf->n_clusters * ivf->dim);
    IVF_TRY(hipSetDevice(ivf->device));
    if (ivf->centroids_host.size() == cents.size()) cents = ivf->centroids_host;
    else
        IVF_TRY(hipMemcpy2D(cents.data(), (size_t)ivf->dim * 4, ivf->centroids->corpus, (size_t)ivf->centroids->ld * 4,
                            (size_t)ivf->dim * 4, ivf->n_clusters, hipMemcpyDeviceToHost));
    if (ivf->assign_host.size() < rows) return set_error(NMN_ERR_STORAGE, "IVF lists are not current");
    PersistHeader h{};
    memcpy(h.magic, "NMNIDX\0\1", 8);
    h.version = 1;
    h.kind = kPersistIvf;
    h.dim = ivf->dim;
    h.rows = rows;
    h.aux = ivf->n_clusters;
    if (fwrite(&h, sizeof h, 1, fp) != 1 || fwrite(cents.data(), 4, cents.size(), fp) != cents.size() ||
        (rows && fwrite(ivf->assign_host.data(), 4, rows, fp) != rows))
        return persist_io_error("cannot write", path);
    return persist_write_shard(ivf->vectors, fp, path);
}

// the section persist_write_ivf wrote, header already read into h
nmn_status persist_read_ivf(FILE* fp, const char* path, const PersistHeader& h, const nmn_index_desc* overrides, nmn_ivf** out) {
    *out = nullptr;
    if (h.kind != kPersistIvf || h.dim == 0 || h.aux == 0 || h.aux > 0xFFFFFFFFull)
        return set_error(NMN_ERR_SERIALIZATION, "not an IVF index file");
    const uint32_t n_clusters = (uint32_t)h.aux;
    {   // what the header announces must be in the file before anything is sized by it
        const long here = ftell(fp);
        long end = -1;
        if (here >= 0 && fseek(fp, 0, SEEK_END) == 0) end = ftell(fp);
        if (here < 0 || end < here || fseek(fp, here, SEEK_SET) != 0) return set_error(NMN_ERR_IO, "IO error: cannot seek in the index file");
        const uint64_t left = (uint64_t)(end - here);
        if ((uint64_t)n_clusters * h.dim > left / 4ull || h.rows > left / 4ull)
            return set_error(NMN_ERR_SERIALIZATION, "index file truncated (centroids / lists)");
    }
    std::vector<float> cents((size_t)n_clusters * h.dim);
    std::vector<uint32_t> assign((size_t)h.rows);
    if (fread(cents.data(), 4, cents.size(), fp) != cents.size() || (h.rows && fread(assign.data(), 4, h.rows, fp) != h.rows))
        return set_error(NMN_ERR_SERIALIZATION, "index file truncated (centroids / lists)");
    for (uint32_t a : assign)
        if (a >= n_clusters) return set_error(NMN_ERR_SERIALIZATION, "index file corrupt: a list id is out of range");
    PersistHeader hv{};
    nmn_status st = persist_read_header(fp, path, &hv);
    if (st != NMN_OK) return st;
    // (the section must announce exactly the payload its shape implies — persist_read_header has checked that many bytes are
    //  in the file — before anything is allocated by that shape: payload_bytes = 0 would pass the size check with any rows)
    if (hv.kind != kPersistFlat || hv.dim != h.dim || hv.rows != h.rows ||
        hv.payload_bytes != hv.rows * (uint64_t)hv.dim * 4ull + hv.rows * 4ull)
        return set_error(NMN_ERR_SERIALIZATION, "index file header is inconsistent");
    nmn_index_desc d{};
    d.dim = h.dim;
    d.flags = overrides ? overrides->flags : 0;
    d.capacity_rows = std::max<uint64_t>(overrides ? overrides->capacity_rows : 0, std::max<uint64_t>(h.rows, 1));
    d.device = overrides ? overrides->device : -1;
    d.cand_cap = overrides ? overrides->cand_cap : 0;
    nmn_ivf* ivf = nullptr;
    st = ivf_new(&d, cents.data(), n_clusters, &ivf);
    if (st != NMN_OK) return st;
    // the vectors: stream the shard section into ivf->vectors (checksum + integrity check of the magnitudes)
    st = persist_read_rows_into(fp, hv, ivf->vectors);
    if (st == NMN_OK && h.rows) {
        hipError_t e = hipSetDevice(ivf->device);
        if (e == hipSuccess) e = hipMemcpy(ivf->assign, assign.data(), (size_t)h.rows * 4, hipMemcpyHostToDevice);
        if (e != hipSuccess) st = set_error_hip(e, "uploading the lists");
    }
    if (st != NMN_OK) {
        const std::string keep = nmn_last_error();
        nmn_ivf_destroy(ivf);
        return set_error(st, keep.c_str());
    }
    ivf->assign_host = std::move(assign);
    ivf->centroids_host = std::move(cents);
    ivf->list_sizes.assign(n_clusters, 0);
    for (uint32_t a : ivf->assign_host) ivf->list_sizes[a]++;
    ivf->list_sizes_rows = h.rows;
    st = ivf_relayout(ivf);  // (the file holds the vectors in id order; the list-major copy is derived like after a build)
    if (st != NMN_OK) {
        nmn_ivf_destroy(ivf);
        return st;
    }
    *out = ivf;
    return NMN_OK;
}
}  // namespace nmn

extern "C" nmn_status nmn_ivf_save(nmn_ivf* ivf, const char* path) {
    if (!ivf || !path) return set_error(NMN_ERR_INVALID_ARGUMENT, "null argument");
    if (ivf->kind != NMN_IVF_FLAT)  // (before the file is created: a refused save leaves nothing behind)
        return set_error(NMN_ERR_CONFIGURATION, "IVF-PQ / IVF-Binary indexes cannot be saved (only IVF-Flat persists its device layout)");
    FILE* fp = fopen(path, "wb");
    if (!fp) return persist_io_error("cannot create", path);
    nmn_status st = persist_write_ivf(ivf, fp, path);
    if (fclose(fp) != 0 && st == NMN_OK) st = persist_io_error("cannot close", path);
    return st;
}

extern "C" nmn_status nmn_ivf_load(const char* path, const nmn_index_desc* overrides, uint64_t max_file_bytes,
                                   uint64_t max_entries, nmn_ivf** out) {
    if (!path || !out) return set_error(NMN_ERR_INVALID_ARGUMENT, "null argument");
    *out = nullptr;
    nmn_status st = persist_check_file_size(path, max_file_bytes, nullptr);
    if (st != NMN_OK) return st;
    FILE* fp = fopen(path, "rb");
    if (!fp) return persist_io_error("cannot open", path);
    PersistHeader h{};
    st = persist_read_header(fp, path, &h);
    if (st == NMN_OK) st = persist_check_entries(h.rows, max_entries);
    if (st == NMN_OK) st = persist_read_ivf(fp, path, h, overrides, out);
    fclose(fp);
    return st;
}
