"""Sparse calls in the request coalescer (docs/hnsw.md §14): nmn_hnsw_search_sparse and nmn_hnsw_search_sparse_multi join the queue of
the other host-buffer searches, and a batch leaves as one launch with a query kind per query.  Whatever batch a call rode in, it must
receive exactly what it receives alone: ids, score bits, counts, rows_scanned, bytes_scanned, sweep_launches and fallback_queries."""
import functools
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

from tests import _hnsw_oracle as ho

pytestmark = pytest.mark.gpu
F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
THREADS, CALLS = 16, 4
KS = (1, 10, 3, 12, 7, 5, 2, 9)
EFS = (None, 5, 50, 200)


def g_cfg(metric):
    from neumann_amd import HNSWConfig
    return HNSWConfig.high_speed().with_distance_metric(metric)


@functools.lru_cache(maxsize=None)
def corpus(name):
    """the generator of test_gpu_hnsw_sparse_query.py.  name = kind:n:dim -> (rows, dense queries).  mix: half the rows have 60 %
    zeros, the others none; queries 80 % zeros."""
    rng = np.random.default_rng(sum(map(ord, name)))
    kind, n, d = name.split(":")
    n, d = int(n), int(d)
    rows = (rng.standard_normal((n, d)) + 2.0 * rng.standard_normal((6, d))[rng.integers(0, 6, n)]).astype(F)
    sparse_rows = rng.random(n) < 0.5
    rows[sparse_rows[:, None] & (rng.random((n, d)) < 0.6)] = 0.0
    if kind == "special":
        for i in range(4, n, 4):
            rows[i] = rows[rng.integers(0, i)]
        rows[::37] = 0.0
    Q = rng.standard_normal((24, d)).astype(F)
    Q[rng.random(Q.shape) < 0.8] = 0.0
    Q[:4] = rows[rng.integers(0, n, 4)]
    return rows, Q


def gpu_index(name, storage, metric):
    from neumann_amd import GpuHnsw
    rows = corpus(name)[0]
    g = GpuHnsw(rows.shape[1], g_cfg(metric), storage=storage, capacity_hint=len(rows) + 64)
    g.insert(rows)
    return g


def run(g, job):
    """a job is (entry, args); -> (ids, scores, counts, (rows_scanned, bytes_scanned, fallback_queries, sweep_launches))"""
    entry, args = job
    ids, sc, cnt, st = getattr(g, entry)(*args, with_stats=True)
    return ids, sc, cnt, (st.rows_scanned, st.bytes_scanned, st.fallback_queries, st.sweep_launches)


def same(a, b):
    return (np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32)) and np.array_equal(a[2], b[2])
            and a[3] == b[3])


def hammer(g, jobs, n_threads):
    """thread t makes the calls t, t + n_threads, ... behind one barrier"""
    out, errs = [None] * len(jobs), []
    start = threading.Barrier(n_threads)

    def work(t):
        try:
            start.wait()
            for j in range(t, len(jobs), n_threads):
                out[j] = run(g, jobs[j])
        except Exception as e:  # noqa: BLE001 - reported below
            errs.append(e)

    th = [threading.Thread(target=work, args=(t,)) for t in range(n_threads)]
    for x in th:
        x.start()
    for x in th:
        x.join()
    assert not errs, errs
    return out


def one(csr, i):
    a, b = int(csr[0][i]), int(csr[0][i + 1])
    return np.array([0, b - a], np.uint64), csr[1][a:b], csr[2][a:b]


def part(csr, lo, hi):
    a, b = int(csr[0][lo]), int(csr[0][hi])
    return (csr[0][lo:hi + 1] - csr[0][lo]).astype(np.uint64), csr[1][a:b], csr[2][a:b]


def sparse_jobs(csr, n):
    """one query each, the thread's own k and ef"""
    nq = len(csr[0]) - 1
    return [("search_sparse", (*one(csr, j % nq), KS[(j % THREADS) % len(KS)], EFS[(j % THREADS) % len(EFS)])) for j in range(n)]


def crowd_jobs(Q, csr, metric_calls):
    """every call kind, k and ef differing from call to call; job j goes to thread j % THREADS"""
    from neumann_amd import ExtendedDistanceMetric as M
    ks5 = np.array([3, 12, 1, 7, 10], np.uint32)
    efs5 = np.array([0, 5, 200, 50, 0], np.uint32)
    kinds = [
        lambda j: ("search", (Q[j % 24], KS[j % len(KS)], EFS[j % len(EFS)])),
        lambda j: ("search_multi", (Q[5:10], ks5, efs5, 12)),
        lambda j: ("search_sparse", (*one(csr, j % 24), KS[(j + 3) % len(KS)], EFS[(j + 1) % len(EFS)])),
        lambda j: ("search_sparse_multi", (*part(csr, 10, 15), ks5[::-1].copy(), efs5, 16)),
        lambda j: ("search_sparse", (*part(csr, 0, 3), 10, 50)),
    ]
    if metric_calls:
        kinds.append(lambda j: ("search_metric_multi", (Q[2:5], np.array([2, 9, 5], np.uint32), [M(0), M(3), M(4)], 10)))
    return [kinds[j % len(kinds)](j) for j in range(THREADS * CALLS)]


def check_crowd(g, jobs, merged=True):
    lone = [run(g, job) for job in jobs]
    b0, c0 = g.coalesce_stats()
    got = hammer(g, jobs, THREADS)
    for j in range(len(jobs)):
        assert same(got[j], lone[j]), (j, jobs[j][0], got[j][3], lone[j][3])
    batches, calls = g.coalesce_stats()
    if merged:
        assert batches - b0 > 0 and calls - c0 >= 2 * (batches - b0), (batches - b0, calls - c0)
    return batches - b0, calls - c0


# ---- 1. sparse callers only -----------------------------------------------------------------------------------------------------------------
def test_sparse_callers_get_their_lone_answers_and_merge():
    name = "mix:300:20"
    with gpu_index(name, "dense", ho.COSINE) as g:
        csr = g.sparse_from_dense(corpus(name)[1])
        check_crowd(g, sparse_jobs(csr, THREADS * CALLS))


# ---- 2. every call kind in one crowd --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("storage,metric", [("dense", ho.COSINE), ("dense", ho.DOT_PRODUCT), ("quantized", ho.COSINE), ("quantized", ho.DOT_PRODUCT)])
def test_every_call_kind_in_one_crowd(storage, metric):
    """dense, multi, metric, sparse and sparse-multi callers with differing k / ef: their batches mix kinds, so they leave as the
    launch with a kind per query (a batch holding a sparse call on these handles and anything else can take no other)"""
    name = "mix:300:33"
    with gpu_index(name, storage, metric) as g:
        Q = corpus(name)[1]
        csr = g.sparse_from_dense(Q)
        jobs = crowd_jobs(Q, csr, metric_calls=storage == "dense")
        # the launch with a kind per query, whatever the crowd does: one call with differing k is always one
        assert same(run(g, jobs[3]), run(g, jobs[3]))
        _, calls = check_crowd(g, jobs)
        assert calls >= 4


# ---- 3. a Euclidean handle: sparse riders are dense walks of to_dense() ---------------------------------------------------------------------
@pytest.mark.parametrize("storage", ["dense", "quantized"])
def test_euclidean_sparse_riders_equal_the_dense_walk(storage):
    name = "mix:300:20"
    with gpu_index(name, storage, ho.EUCLIDEAN) as g:
        Q = corpus(name)[1]
        csr = g.sparse_from_dense(Q)
        jobs = sparse_jobs(csr, THREADS * CALLS)
        for j in range(0, len(jobs), 3):   # dense callers among them
            jobs[j] = ("search", (Q[j % 24], KS[j % len(KS)], EFS[j % len(EFS)]))
        b0, _ = g.coalesce_stats()
        got = hammer(g, jobs, THREADS)
        assert g.coalesce_stats()[0] - b0 > 0
        for j, (entry, args) in enumerate(jobs):
            want = run(g, ("search", (Q[j % 24], *args[-2:])))     # sparse_jobs takes query j % 24 too
            assert same(got[j], want), (j, entry)


# ---- 4. a bad sparse call among good ones ---------------------------------------------------------------------------------------------------
def test_a_bad_sparse_call_among_good_ones_fails_alone():
    from neumann_amd import _capi
    name = "mix:300:20"
    with gpu_index(name, "dense", ho.COSINE) as g:
        csr = g.sparse_from_dense(corpus(name)[1])
        jobs = sparse_jobs(csr, THREADS * CALLS)
        lone = [run(g, job) for job in jobs]
        seen = []
        start = threading.Barrier(2)

        def bad():
            start.wait()
            for _ in range(10):
                for call in (lambda: g.search_sparse([0, 1, 2], [3, 20], [1.0, 1.0], 5),            # position == dim
                             lambda: g.search_sparse_multi([0, 1, 2], [3, 4], [1.0, 1.0], [3, 9], kstride=4),
                             lambda: g.search_sparse_multi([0, 1, 2], [3, 4], [1.0, 1.0], [3, 0], kstride=4)):
                    try:
                        call()
                        seen.append((0, ""))
                    except _capi.NeumannGpuError as e:
                        seen.append((e.status, str(e)))

        def good():
            start.wait()
            good.out = hammer(g, jobs, THREADS)

        th = [threading.Thread(target=bad), threading.Thread(target=good)]
        for x in th:
            x.start()
        for x in th:
            x.join()
        assert [s for s, _ in seen] == [_capi.ERR_INVALID_ARGUMENT, _capi.ERR_INVALID_ARGUMENT, _capi.ERR_INVALID_TOP_K] * 10
        assert all("index 20 out of bounds for dimension 20" in t for _, t in seen[0::3])
        assert all("kstride" in t for _, t in seen[1::3])
        for j in range(len(jobs)):
            assert same(good.out[j], lone[j]), j


# ---- 5. the calls that ride alone -----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def wide(dim, n=64):
    rng = np.random.default_rng(dim)
    rows = rng.standard_normal((n, dim)).astype(F)
    rows[rng.random(rows.shape) < 0.5] = 0.0
    Q = np.zeros((4, dim), dtype=F)
    for i, nnz in enumerate((10, 300, 2200, 40)):
        Q[i, rng.choice(dim, nnz, replace=False)] = rng.standard_normal(nnz).astype(F)
    return rows, Q


@pytest.mark.parametrize("dim,long_only", [(8192, False), (2304, True)])
def test_sparse_callers_that_ride_alone(dim, long_only):
    """Above 4096 dimensions every sparse call on a dense Cosine handle is a batch of its own; at 2304 dimensions only the call
    with a query of more than 2048 entries is.  ONE dense thread rides beside them, so when every sparse call rides alone no
    batch can carry two calls.  Answers and fallback_queries are the lone ones, with the candidate heap made small enough to fill."""
    from neumann_amd import GpuHnsw
    rows, Q = wide(dim)
    with GpuHnsw(dim, g_cfg(ho.COSINE)) as g:
        g.insert(rows)
        g.set_heap_capacity(results=0, candidates=8)
        csr = g.sparse_from_dense(Q)
        long_job = ("search_sparse_multi", (*part(csr, 1, 3), np.array([3, 7], np.uint32), np.array([0, 50], np.uint32), 8))   # 300 and 2200 entries
        short_job = ("search_sparse", (*one(csr, 0), 5, 50))
        dense_job = ("search", (Q[3], 4, None))
        jobs = []
        for c in range(CALLS):
            jobs += [dense_job] + [long_job if (long_only or t % 2) else short_job for t in range(1, 8)]
        lone = [run(g, job) for job in jobs]
        assert any(x[3][2] > 0 for x in lone)                              # (the small heap does fill: fallback_queries is compared for a reason)
        b0, _ = g.coalesce_stats()
        out, errs = [None] * len(jobs), []
        start = threading.Barrier(8)

        def work(t):
            try:
                start.wait()
                for j in range(t, len(jobs), 8):
                    out[j] = run(g, jobs[j])
            except Exception as e:  # noqa: BLE001
                errs.append(e)

        th = [threading.Thread(target=work, args=(t,)) for t in range(8)]
        for x in th:
            x.start()
        for x in th:
            x.join()
        assert not errs, errs
        for j in range(len(jobs)):
            assert same(out[j], lone[j]), (j, jobs[j][0], out[j][3], lone[j][3])
        assert g.coalesce_stats()[0] - b0 == 0
        if long_only:   # ... while short sparse calls at this dimension do share batches
            check_crowd(g, [short_job, dense_job] * 16)


# ---- 6. an insert between two phases --------------------------------------------------------------------------------------------------------
def test_an_insert_between_two_phases():
    name = "mix:300:20"
    with gpu_index(name, "dense", ho.COSINE) as g:
        Q = corpus(name)[1]
        csr = g.sparse_from_dense(Q)
        jobs = crowd_jobs(Q, csr, metric_calls=True)
        before = [run(g, job) for job in jobs]
        check_crowd(g, jobs)
        g.insert(corpus("mix:48:20")[0])
        assert len(g) == 348
        after = [run(g, job) for job in jobs]
        assert any(not same(a, b) for a, b in zip(after, before))          # (the new rows do show up in some answer)
        check_crowd(g, jobs)


# ---- 7. the knobs, each in a fresh child process ----------------------------------------------------------------------------------------------
CHILD = """
import sys, threading, numpy as np
sys.path.insert(0, {root!r})
from tests import test_gpu_hnsw_sparse_coalesce as t
name = "mix:300:20"
out = {{}}
for storage, metric in (("dense", 0), ("quantized", 0), ("dense", 2)):
    with t.gpu_index(name, storage, metric) as g:
        Q = t.corpus(name)[1]
        jobs = t.crowd_jobs(Q, g.sparse_from_dense(Q), metric_calls=False)
        got = t.hammer(g, jobs, t.THREADS)
        for j, o in enumerate(got):
            for i, w in enumerate("isc"):
                out[f"{{storage}}{{metric}}{{w}}{{j}}"] = o[i]
            out[f"{{storage}}{{metric}}t{{j}}"] = np.array(o[3], dtype=np.uint64)
        out[f"{{storage}}{{metric}}stats"] = np.array(g.coalesce_stats())
np.savez({path!r}, **out)
"""


@pytest.mark.parametrize("knob", ["NMN_HNSW_NO_COALESCE", "NMN_HNSW_HOST_SEARCH"])
def test_the_knobs_in_child_processes(tmp_path, knob):
    """NMN_HNSW_NO_COALESCE=1: callers take turns — the same bits and figures, zero batches.  NMN_HNSW_HOST_SEARCH=1: every walk on
    the host — the same bits."""
    path = str(tmp_path / "out.npz")
    r = subprocess.run([sys.executable, "-c", CHILD.format(root=ROOT, path=path)], env=dict(os.environ, **{knob: "1"}),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    out = np.load(path)
    name = "mix:300:20"
    for storage, metric in (("dense", 0), ("quantized", 0), ("dense", 2)):
        tag = f"{storage}{metric}"
        if knob == "NMN_HNSW_NO_COALESCE":
            assert out[tag + "stats"].tolist() == [0, 0]
        with gpu_index(name, storage, metric) as g:
            Q = corpus(name)[1]
            jobs = crowd_jobs(Q, g.sparse_from_dense(Q), metric_calls=False)
            for j, job in enumerate(jobs):
                want = run(g, job)
                got = (out[f"{tag}i{j}"], out[f"{tag}s{j}"], out[f"{tag}c{j}"], tuple(int(x) for x in out[f"{tag}t{j}"]))
                if knob == "NMN_HNSW_HOST_SEARCH":   # the host walk has its own figures (no launches; the reference's count)
                    assert got[3][3] == 0
                    got, want = got[:3] + (None,), want[:3] + (None,)
                assert same(got, want), (tag, j, job[0], got[3], want[3])
