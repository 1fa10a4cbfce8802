// nmn_hnsw_queue.h — the request coalescer in front of the host-buffer HNSW walk (docs/hnsw.md §11): the queue alone, no HIP, so that
// tools/micro/hnsw_queue_mt.cpp can drive it from many threads under -fsanitize=thread / -fsanitize=address with a stand-in batch.
#pragma once
#include <algorithm>
#include <condition_variable>
#include <cstdint>
#include <deque>
#include <mutex>
#include <string>
#include <vector>

#include "neumann_gpu.h"

namespace nmn {

constexpr uint32_t kShareCandMax = 4096;  // a metric call that asks for more candidates than this runs alone: the launch's rows are
                                          // N x max k, and one huge caller must not size them for a thousand others
constexpr uint32_t kBatchQueries = 1024;  // queries a coalesced batch carries at most: four waves per CU, the largest call §6 measured

struct SparseQueries;  // the canonicalised queries of a sparse call (nmn_hnsw_handle.h); the queue only carries the pointer

// One call of nmn_hnsw_search (k1 / ef1), nmn_hnsw_search_multi (k / ef per query), nmn_hnsw_search_metric (xm, one metric; k1 its
// top_k), nmn_hnsw_search_metric_multi (xm, xm_stride 1: a metric per query; k their top_k), nmn_hnsw_search_sparse (sp; k1 / ef1) or
// nmn_hnsw_search_sparse_multi (sp; k / ef per query) or nmn_hnsw_cache_search (xm, filter, threshold; k1 its top_k) on its way through
// the coalescer.
struct HostWalk {
    const float* q = nullptr;
    const SparseQueries* sp = nullptr;  // a sparse call (docs/hnsw.md §14): query i is entry i of *sp, and q is null
    uint32_t nq = 0, k1 = 0, ef1 = 0, kstride = 0;
    const uint32_t* k = nullptr;
    const uint32_t* ef = nullptr;
    uint64_t* out_ids = nullptr;
    float* out_scores = nullptr;
    uint32_t* out_counts = nullptr;
    const nmn_xmetric* xm = nullptr;  // a metric call (docs/hnsw.md §12): k_of(i) is query i's top_k, metric_of(i) its metric
    uint32_t xm_stride = 0;
    bool filter = false;              // a cache call (docs/hnsw.md §16; xm set): the candidate count is the 3k rule's, the ordering keeps
    float threshold = 0.0f;           // only live nodes whose similarity >= threshold
    bool alone = false;               // nobody rides with this call, and it rides with nobody (a metric call with c above kShareCandMax;
                                      // a sparse call whose entries would change the candidate limit of the others, §14)
    uint32_t rescored = 0;            // filled like evals: the largest candidate count re-ranked
    // filled by the leader of the batch this call rode in
    uint64_t evals = 0;
    uint32_t spilled = 0;
    nmn_status st = NMN_OK;
    std::string err;  // text of a failure, for the caller's thread-local nmn_last_error
    bool done = false, lead = false;
    std::condition_variable cv;
    uint32_t k_of(uint32_t i) const { return k ? k[i] : k1; }
    const nmn_xmetric& metric_of(uint32_t i) const { return xm[(size_t)i * xm_stride]; }
    uint32_t ef_of(uint32_t i, uint32_t ef_search) const {  // hnsw.rs:2102
        const uint32_t e = ef ? ef[i] : ef1;
        return std::max<uint32_t>(e ? e : ef_search, k_of(i));
    }
};

struct WalkQueue {
    std::mutex mu;
    bool busy = false;               // a batch is running (or leadership is being handed on)
    std::deque<HostWalk*> waiting;   // arrival order
    uint64_t batches = 0, calls = 0; // batches of >= 2 calls, and the calls in them
};

// queue / lead / ride.  One batch runs at a time.  A call that finds one running waits in `waiting`; when the batch ends, its
// leader makes the oldest waiter the next leader, and that one takes along every call waiting behind it, in arrival order, up to
// kBatchQueries queries.  (A call that does not fit stays first in line for the batch after; so does a call marked `alone`, which
// then leads a batch of one.)  run(batch) -> status is the
// batch's work, batch[0] being the leader's own call; a failure is every call's of the batch: riders get the status and
// last_error()'s text (taken on the leader's thread) in HostWalk::st / err.  Returns this call's status.
template <class Run, class LastError>
nmn_status coalesce_walk(WalkQueue& q, HostWalk& me, Run&& run, LastError&& last_error) {
    std::vector<HostWalk*> batch{&me};
    {
        std::unique_lock<std::mutex> lk(q.mu);
        if (q.busy) {
            q.waiting.push_back(&me);
            me.cv.wait(lk, [&] { return me.done || me.lead; });
            if (me.done) return me.st;
        } else {
            q.busy = true;
        }
        uint32_t total = me.nq;
        while (!me.alone && !q.waiting.empty() && !q.waiting.front()->alone &&
               (uint64_t)total + q.waiting.front()->nq <= kBatchQueries) {
            batch.push_back(q.waiting.front());
            total += q.waiting.front()->nq;
            q.waiting.pop_front();
        }
        if (batch.size() >= 2) {
            q.batches++;
            q.calls += batch.size();
        }
    }
    const nmn_status st = run(batch);
    const std::string err = st == NMN_OK ? std::string() : last_error();
    {
        std::lock_guard<std::mutex> lk(q.mu);
        for (size_t i = 1; i < batch.size(); i++) {
            batch[i]->st = st;
            batch[i]->err = err;
            batch[i]->done = true;
            batch[i]->cv.notify_one();  // under q.mu: the sleeper cannot return (and destroy its request) before this call is over
        }
        if (!q.waiting.empty()) {
            HostWalk* nx = q.waiting.front();
            q.waiting.pop_front();
            nx->lead = true;
            nx->cv.notify_one();  // busy stays set: leadership passes
        } else {
            q.busy = false;
        }
    }
    return st;
}

}  // namespace nmn
