"""Metric calls in the request coalescer (docs/hnsw.md §12): nmn_hnsw_search_metric and nmn_hnsw_search_metric_multi join the queue of
nmn_hnsw_search / nmn_hnsw_search_multi, and a batch leaves as one walk with the re-rank and the ordering behind it carrying kind,
weights and top_k per query.  Whatever batch a call rode in, it must receive exactly what it receives alone: ids, score bits, counts."""
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
N, D, THREADS, CALLS = 2000, 24, 16, 20
TOPS = (1, 10, 50, 100, 5, 6, 64, 200)


def nine():
    from neumann_amd import ExtendedDistanceMetric as M, GeometricConfig
    return [M(k) for k in range(8)] + [M.Composite(GeometricConfig(0.2, 0.7, 0.1))]


@functools.lru_cache(maxsize=None)
def data():
    from neumann_amd import synth_rows
    return synth_rows(0x5EED0031, 0, N, D), synth_rows(0x5EED0032, 0, THREADS * CALLS, D)


def thread_of(j):
    return j % THREADS


def job(Q, j):
    """each thread has its own metric and top_k"""
    t = thread_of(j)
    return Q[j], TOPS[t % len(TOPS)], nine()[t % 9]


@pytest.fixture(scope="module")
def built():
    """(index, jobs, lone answers): 2 000 x 24 built by the library, one job per (thread, call), lone answers taken first"""
    from neumann_amd import GpuHnsw, HNSWConfig
    rows, Q = data()
    jobs = [job(Q, j) for j in range(len(Q))]
    with GpuHnsw(D, HNSWConfig.high_speed().with_distance_metric(1), capacity_hint=N + 64) as g:
        g.insert(rows)
        lone = [g.search_metric(q, k, m) for q, k, m in jobs]
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
                q, k, m = jobs[j]
                out[j] = g.search_metric(q, k, m)
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


def test_concurrent_metric_callers_get_their_lone_answers_and_merge(built):
    g, jobs, lone = built
    b0, c0 = g.coalesce_stats()
    got = hammer(g, jobs, THREADS)
    batches, calls = g.coalesce_stats()
    for j in range(len(jobs)):
        assert same(got[j], lone[j]), (j, jobs[j][1:])
    assert batches - b0 > 0 and calls - c0 >= 2 * (batches - b0), (batches - b0, calls - c0)


def test_every_call_kind_in_one_crowd(built):
    """search, search_multi and search_metric_multi callers among the search_metric threads"""
    g, jobs, lone = built
    Q = data()[1][:9]
    ks = np.array([1, 200, 3, 51, 10, 50, 7, 1, 120], np.uint32)
    efs = np.array([0, 10, 300, 0, 64, 64, 0, 1500, 10], np.uint32)   # one of them beyond the LDS results heap
    tops = np.array([1, 5, 6, 10, 64, 200, 600, 3, 10], np.uint32)    # one of them beyond it too (c = 1 200)
    metrics = nine()
    want = {"plain": g.search(Q[:3], 10), "multi": g.search_multi(Q, ks, efs, kstride=256),
            "mmulti": g.search_metric_multi(Q, tops, metrics, kstride=640)}
    for i in range(len(Q)):                                           # the metric_multi call itself against lone calls
        k = int(tops[i])
        a = g.search_metric(Q[i], k, metrics[i])
        assert np.array_equal(want["mmulti"][0][i, :k], a[0][0]) and want["mmulti"][2][i] == a[2][0]
        assert np.array_equal(want["mmulti"][1][i, :k].view(np.uint32), a[1][0].view(np.uint32))
    res = {"plain": [], "multi": [], "mmulti": []}

    def plain():
        for _ in range(10):
            res["plain"].append(g.search(Q[:3], 10))

    def multi():
        for _ in range(10):
            res["multi"].append(g.search_multi(Q, ks, efs, kstride=256))

    def mmulti():
        for _ in range(10):
            res["mmulti"].append(g.search_metric_multi(Q, tops, metrics, kstride=640))

    got = hammer(g, jobs[:THREADS * 8], THREADS, extra=[plain, multi, mmulti])
    for j in range(THREADS * 8):
        assert same(got[j], lone[j]), j
    for name, r in res.items():
        assert len(r) == 10 and all(same(x, want[name]) for x in r), name


def test_a_bad_call_among_good_ones_fails_alone(built):
    from neumann_amd import ExtendedDistanceMetric as M, _capi
    g, jobs, lone = built
    seen = []

    def bad():
        for _ in range(20):
            for call in (lambda: g.search_metric(np.zeros(D, F), 0, M(0)),                         # top_k == 0
                         lambda: g.search_metric_multi(np.zeros((2, D), F), [3, 9], [M(0), M(1)], kstride=4),
                         lambda: g.search_metric_multi(np.zeros((2, D), F), [3, 3], [M(0), M(9)], kstride=4)):
                try:
                    call()
                except _capi.NeumannGpuError as e:
                    seen.append(e.status)

    got = hammer(g, jobs[:THREADS * 5], THREADS, extra=[bad])
    assert seen == [_capi.ERR_INVALID_TOP_K, _capi.ERR_INVALID_ARGUMENT, _capi.ERR_CONFIGURATION] * 20
    for j in range(THREADS * 5):
        assert same(got[j], lone[j]), j


def test_a_huge_caller_rides_alone():
    """top_k 2 049 on 4 100 rows: c = 4 098 > 4 096, so nobody rides with that call — it gets its lone answer, the uniform chain,
    while the others go on merging"""
    from neumann_amd import GpuHnsw, HNSWConfig, synth_rows
    n, d = 4100, 8
    rows, Q = synth_rows(0x5EED0033, 0, n, d), synth_rows(0x5EED0034, 0, 8 * 10 + 1, d)
    jobs = [(Q[j], TOPS[(j % 8) % len(TOPS)], nine()[(j % 8) % 9]) for j in range(80)]
    with GpuHnsw(d, HNSWConfig.high_speed(), capacity_hint=n) as g:
        g.insert(rows)
        m = nine()[7]
        want = g.search_metric(Q[80], 2049, m)
        lone = [g.search_metric(q, k, mm) for q, k, mm in jobs]
        res = []

        def huge():
            for _ in range(4):
                res.append(g.search_metric(Q[80], 2049, m))

        b0, _ = g.coalesce_stats()
        got = hammer(g, jobs, 8, extra=[huge])
        assert g.coalesce_stats()[0] - b0 > 0
        assert len(res) == 4 and all(same(r, want) for r in res)
        for j in range(len(jobs)):
            assert same(got[j], lone[j]), j


def test_an_insert_between_two_phases(built):
    """LAST test of the module on this handle: it grows the index.  Each phase of callers matches its own lone answers (the candidate
    count c is taken when a batch is launched, under the handle's lock, and the walk sees the rows of that moment)"""
    from neumann_amd import synth_rows
    g, jobs, lone = built
    jobs = jobs[:THREADS * 6]
    got = hammer(g, jobs, THREADS)
    for j in range(len(jobs)):
        assert same(got[j], lone[j]), j
    g.insert(synth_rows(0x5EED0035, 0, 48, D))
    assert len(g) == N + 48
    after = [g.search_metric(q, k, m) for q, k, m in jobs]
    assert any(not same(a, b) for a, b in zip(after, lone))          # (the new rows do show up in some answer)
    got = hammer(g, jobs, THREADS)
    for j in range(len(jobs)):
        assert same(got[j], after[j]), j


def test_the_knob_in_child_process(tmp_path):
    """NMN_HNSW_NO_COALESCE=1 in a fresh child process: callers take turns — the same bits, zero batches"""
    from neumann_amd import GpuHnsw, HNSWConfig, synth_rows
    n, calls = 1500, 6
    code = (
        "import sys, threading, numpy as np\n"
        f"sys.path.insert(0, {ROOT!r})\n"
        "from neumann_amd import GpuHnsw, HNSWConfig, synth_rows, ExtendedDistanceMetric as M, GeometricConfig\n"
        f"n, d, T, calls, TOPS = {n}, {D}, 16, {calls}, {TOPS!r}\n"
        "m9 = [M(k) for k in range(8)] + [M.Composite(GeometricConfig(0.2, 0.7, 0.1))]\n"
        "rows, Q = synth_rows(0x5EED0036, 0, n, d), synth_rows(0x5EED0037, 0, T * calls, d)\n"
        "out = [None] * len(Q)\n"
        "with GpuHnsw(d, HNSWConfig.high_speed()) as g:\n"
        "    g.insert(rows)\n"
        "    start = threading.Barrier(T)\n"
        "    def work(t):\n"
        "        start.wait()\n"
        "        for j in range(t, len(Q), T):\n"
        "            out[j] = g.search_metric(Q[j], TOPS[t % len(TOPS)], m9[t % 9])\n"
        "    th = [threading.Thread(target=work, args=(t,)) for t in range(T)]\n"
        "    [x.start() for x in th]\n"
        "    [x.join() for x in th]\n"
        "    assert all(o is not None for o in out)\n"
        "    stats = g.coalesce_stats()\n"
        f"np.savez({str(tmp_path)!r} + '/out.npz', stats=np.array(stats), **{{f'{{w}}{{j}}': o[i] for j, o in enumerate(out) for i, w in enumerate('isc')}})\n"
    )
    env = dict(os.environ, NMN_HNSW_NO_COALESCE="1")
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    out = np.load(tmp_path / "out.npz")
    assert out["stats"].tolist() == [0, 0]
    rows, Q = synth_rows(0x5EED0036, 0, n, D), synth_rows(0x5EED0037, 0, 16 * calls, D)
    m9 = nine()
    with GpuHnsw(D, HNSWConfig.high_speed()) as g:
        g.insert(rows)
        for j in range(len(Q)):
            t = j % 16
            assert same(g.search_metric(Q[j], TOPS[t % len(TOPS)], m9[t % 9]), (out[f"i{j}"], out[f"s{j}"], out[f"c{j}"])), j
