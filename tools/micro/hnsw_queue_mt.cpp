// hnsw_queue_mt.cpp — the HNSW request coalescer's queue (neumann_amd/csrc/nmn_hnsw_queue.h) driven from many threads with a
// stand-in for the batch, no GPU.  Built for the thread and address sanitizers:
//
//   c++ -std=c++17 -O1 -g -fsanitize=thread  -I include -I neumann_amd/csrc tools/micro/hnsw_queue_mt.cpp -o tools/micro/hnsw_queue_mt -lpthread && tools/micro/hnsw_queue_mt
//   c++ -std=c++17 -O1 -g -fsanitize=address -I include -I neumann_amd/csrc tools/micro/hnsw_queue_mt.cpp -o tools/micro/hnsw_queue_mt -lpthread && tools/micro/hnsw_queue_mt
//
// The stand-in checks what the queue promises: one batch at a time; at most kBatchQueries queries in a batch unless it is one
// call; a call marked `alone` (a metric call with more than kShareCandMax candidates, a sparse call that would change the others'
// candidate limit) is a batch of one; every call is served exactly once, with its own answer (out_counts[i] = a function of the
// call's own k and query), also when a batch fails — then every call of that batch gets the status and the text.  About one call in
// five is a sparse one: HostWalk::sp set and q null, as nmn_hnsw_search_sparse[_multi] submit them; the stand-in batch reads such a
// call's queries through sp and requires q to be null, and sparse and dense calls share batches.  About one call in ten is a cache
// call (docs/hnsw.md §16): HostWalk::xm, filter and threshold set as nmn_hnsw_cache_search submits them; the stand-in batch requires
// the flag to come with a metric and dense queries, and checks that the threshold it reads is the one the caller wrote for that call.
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <thread>

#include "nmn_hnsw_queue.h"

// the queue carries a pointer to the call's canonicalised sparse queries and never looks inside: a stand-in with one value per query
struct nmn::SparseQueries {
    std::vector<float> v;
};

using namespace nmn;

static std::atomic<int> running{0};
static std::atomic<uint64_t> batches_run{0}, calls_served{0}, failed_batches{0}, alone_served{0}, sparse_served{0}, mixed_batches{0}, cache_served{0}, cache_mixed{0};
static thread_local std::string tl_error;

#define REQUIRE(c)                                                   \
    do {                                                             \
        if (!(c)) {                                                  \
            fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
            abort();                                                 \
        }                                                            \
    } while (0)

static nmn_status fake_batch(const std::vector<HostWalk*>& batch) {
    REQUIRE(running.fetch_add(1) == 0);  // one batch at a time
    uint64_t total = 0;
    for (const HostWalk* r : batch) total += r->nq;
    REQUIRE(batch.size() == 1 || total <= kBatchQueries);
    for (const HostWalk* r : batch)
        if (r->alone) {  // nobody rides with it, and it rides with nobody
            REQUIRE(batch.size() == 1);
            alone_served++;
        }
    size_t sparse_here = 0;
    for (const HostWalk* r : batch) {
        REQUIRE(!r->sp != !r->q);  // a call brings dense queries or sparse ones, never both
        if (r->sp) {
            REQUIRE(r->sp->v.size() == r->nq);
            sparse_here++;
        }
    }
    sparse_served += sparse_here;
    size_t cache_here = 0;
    for (const HostWalk* r : batch) {
        if (!r->filter) continue;
        REQUIRE(r->xm && r->q && !r->sp);                              // a cache call is a metric call with dense queries
        REQUIRE(r->threshold == 0.5f + (float)((uint32_t)r->q[0] % 7));  // ... and carries its own threshold
        cache_here++;
    }
    cache_served += cache_here;
    if (cache_here && cache_here < batch.size()) cache_mixed++;
    if (sparse_here && sparse_here < batch.size()) mixed_batches++;
    const uint64_t b = batches_run.fetch_add(1);
    nmn_status st = NMN_OK;
    if (b % 17 == 5) {  // a failing batch: nothing written, every call gets the status
        tl_error = "batch " + std::to_string(b) + " failed";
        failed_batches++;
        st = NMN_ERR_INVALID_ARGUMENT;
    } else {
        for (HostWalk* r : batch) {
            for (uint32_t i = 0; i < r->nq; i++) r->out_counts[i] = r->k_of(i) * 1000u + (uint32_t)(r->sp ? r->sp->v[i] : r->q[i]);
            r->evals = r->nq;
        }
    }
    std::this_thread::sleep_for(std::chrono::microseconds(50 + (b % 5) * 40));
    calls_served += batch.size();
    REQUIRE(running.fetch_sub(1) == 1);
    return st;
}

int main() {
    const int threads = 24, calls = 400;
    WalkQueue q;
    std::atomic<uint64_t> failures_seen{0};
    std::vector<std::thread> th;
    for (int t = 0; t < threads; t++) {
        th.emplace_back([&, t] {
            for (int c = 0; c < calls; c++) {
                const uint32_t nq = (t == 0 && c % 50 == 0) ? 1500u : 1u + (uint32_t)((t + c) % 7 == 0 ? 300 : (t + c) % 3);  // some calls larger than a batch
                std::vector<float> query(nq);
                std::vector<uint32_t> k(nq), counts(nq, 0xFFFFFFFFu);
                for (uint32_t i = 0; i < nq; i++) {
                    query[i] = (float)((t * 31 + c + i) % 997);
                    k[i] = 1 + (uint32_t)((t + c + i) % 200);
                }
                HostWalk me;
                SparseQueries sq;
                if ((t * 3 + c) % 5 == 1) {  // a sparse call: its queries behind sp, q null
                    sq.v = query;
                    me.sp = &sq;
                } else {
                    me.q = query.data();
                }
                const nmn_xmetric cosine{NMN_XMETRIC_COSINE, 0.0f, 0.0f, 0.0f};
                if (!me.sp && (t * 5 + c) % 10 == 4) {  // a cache call: a metric, the filter flag and a threshold of its own
                    me.xm = &cosine;
                    me.filter = true;
                    me.threshold = 0.5f + (float)((uint32_t)query[0] % 7);
                }
                me.nq = nq;
                me.k = k.data();
                me.kstride = 200;
                me.out_counts = counts.data();
                me.alone = (t * 7 + c) % 11 == 3;  // the calls that ride alone, from every thread
                const nmn_status st = coalesce_walk(q, me, fake_batch, [] { return tl_error; });
                if (st == NMN_OK) {
                    REQUIRE(me.evals == nq || me.done);  // (a rider's evals are written by the leader before done is set)
                    for (uint32_t i = 0; i < nq; i++) REQUIRE(counts[i] == k[i] * 1000u + (uint32_t)query[i]);
                } else {
                    REQUIRE(st == NMN_ERR_INVALID_ARGUMENT);
                    if (me.done) REQUIRE(me.err.find("failed") != std::string::npos);  // a rider carries the leader's text
                    for (uint32_t i = 0; i < nq; i++) REQUIRE(counts[i] == 0xFFFFFFFFu);
                    failures_seen++;
                }
            }
        });
    }
    for (auto& x : th) x.join();
    REQUIRE(calls_served.load() == (uint64_t)threads * calls);
    REQUIRE(!q.busy && q.waiting.empty());
    REQUIRE(q.batches > 0 && q.calls >= 2 * q.batches);
    REQUIRE(failed_batches.load() > 0 && failures_seen.load() >= failed_batches.load());
    uint64_t alone_made = 0;
    for (int t = 0; t < threads; t++)
        for (int c = 0; c < calls; c++) alone_made += (t * 7 + c) % 11 == 3 ? 1 : 0;
    REQUIRE(alone_made > 0 && alone_served.load() == alone_made);
    uint64_t sparse_made = 0;
    for (int t = 0; t < threads; t++)
        for (int c = 0; c < calls; c++) sparse_made += (t * 3 + c) % 5 == 1 ? 1 : 0;
    REQUIRE(sparse_made > 0 && sparse_served.load() == sparse_made && mixed_batches.load() > 0);
    uint64_t cache_made = 0;
    for (int t = 0; t < threads; t++)
        for (int c = 0; c < calls; c++) cache_made += ((t * 3 + c) % 5 != 1 && (t * 5 + c) % 10 == 4) ? 1 : 0;
    REQUIRE(cache_made > 0 && cache_served.load() == cache_made && cache_mixed.load() > 0);
    printf("hnsw_queue_mt cache calls: %llu, in %llu batches with other kinds of call\n", (unsigned long long)cache_made,
           (unsigned long long)cache_mixed.load());
    printf("hnsw_queue_mt ok: %llu calls in %llu batches (%llu merged batches carrying %llu calls, %llu calls alone, %llu sparse calls, %llu batches mixing sparse and dense calls), %llu failed batches, %llu failed calls\n",
           (unsigned long long)calls_served.load(), (unsigned long long)batches_run.load(), (unsigned long long)q.batches,
           (unsigned long long)q.calls, (unsigned long long)alone_served.load(), (unsigned long long)sparse_served.load(),
           (unsigned long long)mixed_batches.load(), (unsigned long long)failed_batches.load(), (unsigned long long)failures_seen.load());
    return 0;
}
