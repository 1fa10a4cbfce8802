"""Cache calls in the request coalescer (docs/hnsw.md §16): nmn_hnsw_cache_search joins the queue of every other host-buffer search, and
a batch leaves as one walk with the re-rank, the merge re-rank of Sparse-node candidates and the filtered ordering behind it carrying
kind, weights, top_k, threshold and the filter flag per query.  Whatever batch a call rode in, it must receive exactly what it
receives alone: ids, similarity bits, counts.  (The lone answers are held to the oracle in tests/test_gpu_hnsw_cache_search.py.)"""
import functools
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, D, THREADS, CALLS = 1500, 24, 16, 12
KS = (1, 4, 2, 10, 1, 7, 3, 40)
THRS = (0.9, 0.1, -np.inf, 0.3, 0.5, 0.0, 0.05, 0.2)


def nine():
    from neumann_amd import ExtendedDistanceMetric as M, GeometricConfig
    return [M(k) for k in range(8)] + [M.Composite(GeometricConfig(0.2, 0.7, 0.1))]


def fill(g, seed=0):
    """1 000 Dense rows, 500 Sparse ones (60 % zeros), eight of them with a duplicated position; a seventh of the nodes dead"""
    from neumann_amd import synth_rows
    rows = synth_rows(0x5EED0041 + seed, 0, N, D)
    g.insert(rows[:1000])
    sp = rows[1000:].copy()
    sp[np.random.default_rng(41).random(sp.shape) < 0.6] = 0.0
    indptr, pos, val = g.sparse_from_dense(sp)
    g.insert_sparse(indptr[:493], pos[:int(indptr[492])], val[:int(indptr[492])])
    for i in range(492, 500):                                     # one stored position once more, with another value
        a, b = int(indptr[i]), int(indptr[i + 1])
        p, v = list(pos[a:b]) + [pos[a]], list(val[a:b]) + [F(0.75)]
        g.insert_sparse([0, len(p)], p, v)
    g.set_node_mask(np.arange(0, N, 7), False)
    return rows


@functools.lru_cache(maxsize=None)
def queries():
    from neumann_amd import synth_rows
    return synth_rows(0x5EED0042, 0, THREADS * CALLS, D)


def job(Q, j):
    """each thread has its own k, threshold and metric"""
    t = j % THREADS
    return Q[j], KS[t % len(KS)], THRS[(t // 2) % len(THRS)], nine()[t % 9]


@pytest.fixture(scope="module")
def built():
    from neumann_amd import GpuHnsw, HNSWConfig
    Q = queries()
    jobs = [job(Q, j) for j in range(len(Q))]
    with GpuHnsw(D, HNSWConfig.high_speed(), capacity_hint=N + 64) as g:
        fill(g)
        lone = [g.cache_search(q, k, thr, m) for q, k, thr, m in jobs]
        assert sum(int(a[2][0]) for a in lone) > len(jobs) // 2 and any(int(a[2][0]) < k for a, (_, k, _, _) in zip(lone, jobs))
        yield g, jobs, lone


def same(a, b):
    return (np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))
            and np.array_equal(a[2], b[2]))


def hammer(g, jobs, n_threads, extra=()):
    """thread t makes the calls t, t + n_threads, ...; `extra`: further thread bodies started behind the same barrier"""
    out = [None] * len(jobs)
    errs = []
    start = threading.Barrier(n_threads + len(extra))

    def work(t):
        try:
            start.wait()
            for j in range(t, len(jobs), n_threads):
                q, k, thr, m = jobs[j]
                out[j] = g.cache_search(q, k, thr, m, with_stats=True)
        except Exception as e:  # noqa: BLE001 - reported below
            errs.append(e)

    def other(f):
        try:
            start.wait()
            f()
        except Exception as e:  # noqa: BLE001
            errs.append(e)

    th = [threading.Thread(target=work, args=(t,)) for t in range(n_threads)] + [threading.Thread(target=other, args=(f,)) for f in extra]
    for x in th:
        x.start()
    for x in th:
        x.join()
    assert not errs, errs
    return out


def test_sixteen_cache_callers_get_their_lone_answers_and_merge(built):
    g, jobs, lone = built
    lone_stats = [g.cache_search(q, k, thr, m, with_stats=True)[3] for q, k, thr, m in jobs[:THREADS]]
    b0, c0 = g.coalesce_stats()
    got = hammer(g, jobs, THREADS)
    batches, calls = g.coalesce_stats()
    for j in range(len(jobs)):
        assert same(got[j], lone[j]), (j, jobs[j][1:])
    assert batches - b0 > 0 and calls - c0 >= 2 * (batches - b0), (batches - b0, calls - c0)
    for j in range(THREADS):   # a call's stats are its own, whatever batch it rode in
        assert got[j][3].rows_scanned == lone_stats[j].rows_scanned and got[j][3].candidates_rescored == lone_stats[j].candidates_rescored
    # ... and a call of several queries sums the walk's figures of its queries
    q3 = np.stack([jobs[0][0], jobs[16][0], jobs[32][0]])
    one = g.cache_search(q3, 1, 0.9, nine()[0], with_stats=True)
    parts = [g.cache_search(q, 1, 0.9, nine()[0], with_stats=True) for q in q3]
    assert one[3].rows_scanned == sum(p[3].rows_scanned for p in parts)
    assert one[3].candidates_rescored == max(p[3].candidates_rescored for p in parts) == 10
    for i, p in enumerate(parts):
        assert np.array_equal(one[0][i], p[0][0]) and one[2][i] == p[2][0]


def test_every_call_kind_in_one_crowd(built):
    """search, search_multi, search_metric, search_metric_multi, search_sparse and cache_search_sparse callers among the cache threads"""
    g, jobs, lone = built
    Q = queries()[:9]
    ks = np.array([1, 200, 3, 51, 10, 50, 7, 1, 120], np.uint32)
    tops = np.array([1, 5, 6, 10, 64, 200, 3, 3, 10], np.uint32)
    metrics = nine()
    sp = Q[:4].copy()
    sp[:, ::2] = 0.0
    csr = g.sparse_from_dense(sp)
    calls = {"plain": lambda: g.search(Q[:3], 10), "multi": lambda: g.search_multi(Q, ks, kstride=256),
             "metric": lambda: g.search_metric(Q[:2], 5, metrics[6]),
             "mmulti": lambda: g.search_metric_multi(Q, tops, metrics, kstride=256),
             "sparse": lambda: g.search_sparse(*csr, 10),
             "csparse": lambda: g.cache_search_sparse(*csr, 4, 0.1, metrics[5])}
    want = {name: f() for name, f in calls.items()}
    res = {name: [] for name in calls}

    def body(name):
        def run():
            for _ in range(8):
                res[name].append(calls[name]())
        return run

    got = hammer(g, jobs[:THREADS * 8], THREADS, extra=[body(n) for n in calls])
    for j in range(THREADS * 8):
        assert same(got[j], lone[j]), j
    for name, r in res.items():
        assert len(r) == 8 and all(same(x, want[name]) for x in r), name


def test_a_bad_call_among_good_ones_fails_alone(built):
    from neumann_amd import ExtendedDistanceMetric as M, _capi
    g, jobs, lone = built
    seen = []

    def bad():
        for _ in range(20):
            for call in (lambda: g.cache_search(np.zeros(D, F), 0, 0.5, M(0)),     # k == 0
                         lambda: g.cache_search(np.zeros(D, F), 3, 0.5, M(9)),     # an unknown kind
                         lambda: g.cache_search_sparse([0, 1], [D], [1.0], 3, 0.5, M(0))):
                try:
                    call()
                except _capi.NeumannGpuError as e:
                    seen.append(e.status)

    got = hammer(g, jobs[:THREADS * 5], THREADS, extra=[bad])
    assert seen == [_capi.ERR_INVALID_TOP_K, _capi.ERR_CONFIGURATION, _capi.ERR_INVALID_ARGUMENT] * 20
    for j in range(THREADS * 5):
        assert same(got[j], lone[j]), j


def test_a_mask_change_between_two_phases(built):
    """LAST test of the module on this handle: it flips bits.  Each phase of callers matches its own lone answers"""
    g, jobs, lone = built
    jobs = jobs[:THREADS * 6]
    got = hammer(g, jobs, THREADS)
    for j in range(len(jobs)):
        assert same(got[j], lone[j]), j
    top = [int(a[0][0, 0]) for a in lone[:len(jobs)] if a[2][0] > 0]
    g.set_node_mask(top, False)                                     # the best answers die ...
    g.set_node_mask(np.arange(0, N, 14), True)                      # ... and half of the dead come back
    after = [g.cache_search(q, k, thr, m) for q, k, thr, m in jobs]
    assert any(not same(a, b) for a, b in zip(after, lone))
    assert all(int(a[0][0, 0]) not in top for a in after if a[2][0] > 0)
    got = hammer(g, jobs, THREADS)
    for j in range(len(jobs)):
        assert same(got[j], after[j]), j


@pytest.mark.parametrize("knob", ["NMN_HNSW_NO_COALESCE", "NMN_HNSW_HOST_SEARCH", "NMN_XMETRIC_SORT_FROM"])
def test_the_knobs_in_a_child_process(tmp_path, knob):
    """a fresh child process under the knob: the same bits; without the coalescer zero batches; with the host walk no launch; with
    NMN_XMETRIC_SORT_FROM=8 every cache query of the merged batches (differing k, threshold and metric: the per-query launches) is
    ordered by the filtered prep kernel and the large-k sort, against this process's rank path"""
    from neumann_amd import GpuHnsw, HNSWConfig
    calls = 4
    code = (
        "import sys, threading, numpy as np\n"
        f"sys.path.insert(0, {ROOT!r})\n"
        "from neumann_amd import GpuHnsw, HNSWConfig\n"
        "from tests import test_gpu_hnsw_cache_coalesce as t\n"
        f"T, calls = 16, {calls}\n"
        "Q = t.queries()[:T * calls]\n"
        "out = [None] * len(Q)\n"
        "with GpuHnsw(t.D, HNSWConfig.high_speed()) as g:\n"
        "    t.fill(g, 1)\n"
        "    start = threading.Barrier(T)\n"
        "    def work(th):\n"
        "        start.wait()\n"
        "        for j in range(th, len(Q), T):\n"
        "            q, k, thr, m = t.job(Q, j)\n"
        "            out[j] = g.cache_search(q, k, thr, m, with_stats=True)\n"
        "    ths = [threading.Thread(target=work, args=(i,)) for i in range(T)]\n"
        "    [x.start() for x in ths]\n"
        "    [x.join() for x in ths]\n"
        "    assert all(o is not None for o in out)\n"
        "    stats = g.coalesce_stats()\n"
        "launches = np.array([o[3].sweep_launches for o in out])\n"
        f"np.savez({str(tmp_path)!r} + '/out.npz', stats=np.array(stats), launches=launches, "
        "**{f'{w}{j}': o[i] for j, o in enumerate(out) for i, w in enumerate('isc')})\n"
    )
    env = dict(os.environ, **{knob: "8" if knob == "NMN_XMETRIC_SORT_FROM" else "1"})
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    out = np.load(tmp_path / "out.npz")
    if knob == "NMN_HNSW_NO_COALESCE":
        assert out["stats"].tolist() == [0, 0]
    elif knob == "NMN_HNSW_HOST_SEARCH":
        assert (out["launches"] == 0).all()
    else:
        assert out["stats"][0] > 0 and out["stats"][1] >= 2 * out["stats"][0]   # (merged batches did carry these calls)
    Q = queries()[:16 * calls]
    with GpuHnsw(D, HNSWConfig.high_speed()) as g:
        fill(g, 1)
        for j in range(len(Q)):
            q, k, thr, m = job(Q, j)
            assert same(g.cache_search(q, k, thr, m), (out[f"i{j}"], out[f"s{j}"], out[f"c{j}"])), j
