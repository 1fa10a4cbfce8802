"""The request coalescer in front of nmn_hnsw_search / nmn_hnsw_search_multi (docs/hnsw.md §11): calls that arrive while a walk of
the handle is running leave together as one launch with a k and an ef per query.  Whatever batch a call rode in, it must receive
exactly what it receives alone: ids, score bits, counts."""
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
N, D, THREADS, CALLS = 20_000, 32, 32, 20
KS = (1, 3, 10, 50, 51, 200)
EFS = (None, 10, 64, 300)


@functools.lru_cache(maxsize=None)
def data():
    from neumann_amd import synth_rows
    return synth_rows(0x5EED0021, 0, N, D), synth_rows(0x5EED0022, 0, THREADS * CALLS, D)


@pytest.fixture(scope="module")
def built():
    """(index, jobs, lone answers): 20 000 x 32 built by the library, one job per (thread, call), lone answers taken first"""
    from neumann_amd import GpuHnsw, HNSWConfig
    rows, Q = data()
    jobs = [(Q[j], KS[j % len(KS)], EFS[(j // 3) % len(EFS)]) for j in range(len(Q))]
    with GpuHnsw(D, HNSWConfig.high_speed().with_distance_metric(1), capacity_hint=N + 64) as g:
        g.insert(rows)
        lone = [g.search(q, k, ef) for q, k, ef in jobs]
        yield g, jobs, lone


def same(a, b):
    return (np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))
            and np.array_equal(a[2], b[2]))


def hammer(g, jobs, n_threads, extra=()):
    """thread t walks jobs t, t + n_threads, ...; `extra`: further thread bodies started behind the same barrier"""
    out = [None] * len(jobs)
    errs = []
    start = threading.Barrier(n_threads + len(extra))

    def work(t):
        try:
            start.wait()
            for j in range(t, len(jobs), n_threads):
                q, k, ef = jobs[j]
                out[j] = g.search(q, k, ef)
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


def test_concurrent_callers_get_their_lone_answers(built):
    g, jobs, lone = built
    b0, c0 = g.coalesce_stats()
    got = hammer(g, jobs, THREADS)
    batches, calls = g.coalesce_stats()
    for j in range(len(jobs)):
        assert same(got[j], lone[j]), (j, jobs[j][1:])
    assert batches - b0 > 0 and calls - c0 >= 2 * (batches - b0), (batches - b0, calls - c0)


def test_a_bad_call_among_good_ones_fails_alone(built):
    from neumann_amd import _capi
    g, jobs, lone = built
    seen = []

    def bad():
        for _ in range(20):
            try:
                g.search(np.zeros(D, F), 0)                  # k == 0: refused before it can join a batch
            except _capi.NeumannGpuError as e:
                seen.append(e.status)
            try:
                g.search_multi(np.zeros((2, D), F), [3, 9], kstride=4)
            except _capi.NeumannGpuError as e:
                seen.append(e.status)

    got = hammer(g, jobs[:THREADS * 5], THREADS, extra=[bad])
    assert seen == [_capi.ERR_INVALID_TOP_K, _capi.ERR_INVALID_ARGUMENT] * 20
    for j in range(THREADS * 5):
        assert same(got[j], lone[j]), j


def test_mixed_call_kinds(built):
    """a search_multi caller (several queries, its own kstride) and a search_metric caller (which takes its turn between batches)
    among the threads"""
    from neumann_amd.xmetric import ExtendedDistanceMetric
    g, jobs, lone = built
    Q = data()[1][:9]
    ks = np.array([1, 200, 3, 51, 10, 50, 7, 1, 120], np.uint32)
    efs = np.array([0, 10, 300, 0, 64, 64, 0, 1500, 10], np.uint32)   # one of them beyond the LDS results heap
    metric = ExtendedDistanceMetric.from_name("manhattan")
    want_multi = g.search_multi(Q, ks, efs, kstride=256)
    want_metric = g.search_metric(Q[:3], 10, metric)
    res = {"multi": [], "metric": []}

    def multi():
        for _ in range(10):
            res["multi"].append(g.search_multi(Q, ks, efs, kstride=256))

    def by_metric():
        for _ in range(10):
            res["metric"].append(g.search_metric(Q[:3], 10, metric))

    got = hammer(g, jobs[:THREADS * 8], THREADS, extra=[multi, by_metric])
    for j in range(THREADS * 8):
        assert same(got[j], lone[j]), j
    assert len(res["multi"]) == 10 and all(same(r, want_multi) for r in res["multi"])
    assert len(res["metric"]) == 10 and all(same(r, want_metric) for r in res["metric"])
    for i in range(len(Q)):                                  # and the multi call itself against lone calls
        k = int(ks[i])
        a = g.search(Q[i], k, int(efs[i]))
        assert np.array_equal(want_multi[0][i, :k], a[0][0]) and want_multi[2][i] == a[2][0]
        assert np.array_equal(want_multi[1][i, :k].view(np.uint32), a[1][0].view(np.uint32))


def test_an_insert_in_the_middle(built):
    """LAST test of the module on this handle: it grows the index.  Every answer equals the lone answer before the insert or the
    lone answer after it."""
    from neumann_amd import synth_rows
    g, jobs, lone = built
    jobs = jobs[:THREADS * 10]
    extra_rows = synth_rows(0x5EED0023, 0, 48, D)

    def insert():
        g.insert(extra_rows)

    got = hammer(g, jobs, THREADS, extra=[insert])
    assert len(g) == N + 48
    after = [g.search(q, k, ef) for q, k, ef in jobs]
    for j in range(len(jobs)):
        assert same(got[j], lone[j]) or same(got[j], after[j]), j


def test_the_knob_in_child_process(tmp_path):
    """NMN_HNSW_NO_COALESCE=1 in a fresh child process: callers take turns — the same bits, zero batches"""
    from neumann_amd import GpuHnsw, HNSWConfig, synth_rows
    n, calls = 3000, 6
    code = (
        "import sys, threading, numpy as np\n"
        f"sys.path.insert(0, {ROOT!r})\n"
        "from neumann_amd import GpuHnsw, HNSWConfig, synth_rows\n"
        f"n, d, T, calls, KS = {n}, {D}, 16, {calls}, {KS!r}\n"
        "rows, Q = synth_rows(0x5EED0024, 0, n, d), synth_rows(0x5EED0025, 0, T * calls, d)\n"
        "out = [None] * len(Q)\n"
        "with GpuHnsw(d, HNSWConfig.high_speed()) as g:\n"
        "    g.insert(rows)\n"
        "    start = threading.Barrier(T)\n"
        "    def work(t):\n"
        "        start.wait()\n"
        "        for j in range(t, len(Q), T):\n"
        "            out[j] = g.search(Q[j], KS[j % len(KS)])\n"
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
    rows, Q = synth_rows(0x5EED0024, 0, n, D), synth_rows(0x5EED0025, 0, 16 * calls, D)
    with GpuHnsw(D, HNSWConfig.high_speed()) as g:
        g.insert(rows)
        for j in range(len(Q)):
            assert same(g.search(Q[j], KS[j % len(KS)]), (out[f"i{j}"], out[f"s{j}"], out[f"c{j}"])), j
