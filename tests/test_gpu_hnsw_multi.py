"""nmn_hnsw_search_multi (GpuHnsw.search_multi): one launch that carries a k and an ef per query.  The answer for query i must be
bit for bit what nmn_hnsw_search(q_i, 1, k[i], ef[i]) returns alone — ids, score bits, counts, and the distance evaluations and
spill-launch figures of the stats — on dense and quantized handles, on both sides of the LDS limit and through both overflow
paths.  The lone call is the uniform kernel, which tests/test_gpu_hnsw.py and tests/test_gpu_hnsw_q8.py hold to the oracle; the
golden corpus ties the mixed launch to the oracle's frozen answers directly."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "hnsw_small.npz")
U64_MAX = np.uint64(0xFFFFFFFFFFFFFFFF)
METRICS = [0, 1, 2]                      # Cosine, Euclidean, DotProduct
STORAGES = ["dense", "quantized"]
KS = (1, 3, 10, 50, 51, 200)             # 50 / 51: either side of ef_search, where ef = max(ef, k) starts to follow k
EFS = (0, 10, 64, 300)                   # 0 = ef_search


@functools.lru_cache(maxsize=None)
def corpus(n, d):
    """clustered rows, a quarter of them exact duplicates of earlier ones (ties have to be decided); 40 queries, 10 of them rows"""
    rng = np.random.default_rng(1000 * n + d)
    rows = (rng.standard_normal((n, d)) + 2.0 * rng.standard_normal((6, d))[rng.integers(0, 6, n)]).astype(F)
    for i in range(4, n, 4):
        rows[i] = rows[rng.integers(0, i)]
    queries = rng.standard_normal((40, d)).astype(F)
    if n:
        queries[:10] = rows[rng.integers(0, n, 10)]
    return rows, queries


def index(n, d, metric, storage, preset="default"):
    from neumann_amd import GpuHnsw, HNSWConfig
    g = GpuHnsw(d, getattr(HNSWConfig, preset)().with_distance_metric(metric), storage=storage)
    if n:
        g.insert(corpus(n, d)[0])
    return g


def mixed(nq, seed):
    """k and ef per query, every value of KS and EFS present when nq allows"""
    rng = np.random.default_rng(seed)
    ks = np.array([KS[i % len(KS)] for i in range(nq)], np.uint32)
    efs = np.array([EFS[(i // 2) % len(EFS)] for i in range(nq)], np.uint32)
    rng.shuffle(ks)
    return ks, efs


def assert_multi_equals_lone(g, Q, ks, efs, kstride=None):
    """one search_multi call against one lone search call per query; returns the multi call's stats"""
    ids, sc, cnt, st = g.search_multi(Q, ks, efs, kstride=kstride, with_stats=True)
    kstride = int(max(ks)) if kstride is None else kstride
    assert ids.shape == sc.shape == (len(Q), kstride)
    evals = spilled = 0
    for i in range(len(Q)):
        k = int(ks[i])
        li, ls, lc, lst = g.search(Q[i], k, None if efs is None else int(efs[i]), with_stats=True)
        assert cnt[i] == lc[0], (i, k, cnt[i], lc[0])
        assert np.array_equal(ids[i, :k], li[0]), (i, k)
        assert np.array_equal(sc[i, :k].view(np.uint32), ls[0].view(np.uint32)), (i, k)
        assert np.all(ids[i, cnt[i]:] == U64_MAX) and np.all(np.isneginf(sc[i, cnt[i]:])), (i, k)
        evals += lst.rows_scanned
        spilled += lst.fallback_queries
    assert st.rows_scanned == evals, (st.rows_scanned, evals)
    assert st.fallback_queries == spilled, (st.fallback_queries, spilled)
    return st


@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("n,d", [(2000, 20), (300, 5), (300, 33)])
def test_mixed_k_and_ef_in_one_call(n, d, metric, storage):
    Q = corpus(n, d)[1]
    ks, efs = mixed(len(Q), 7)
    with index(n, d, metric, storage) as g:
        st = assert_multi_equals_lone(g, Q, ks, efs)
        assert st.fallback_queries == 0
        assert_multi_equals_lone(g, Q, ks, None)                    # ef NULL: ef_search for every query


@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("metric", METRICS)
def test_a_call_split_between_the_two_first_launches(metric, storage):
    """one query at ef 1 500: its results heap (1 501 entries) does not fit LDS and it goes straight to the spill launch, the
    others start in LDS — the call is split and reassembled in the caller's order"""
    Q = corpus(2000, 20)[1]
    ks, efs = mixed(len(Q), 11)
    efs[17] = 1500
    with index(2000, 20, metric, storage) as g:
        st = assert_multi_equals_lone(g, Q, ks, efs)
        assert st.fallback_queries == 1
        efs[[0, 39]] = 1200, 1500                                   # the first and the last of the call too
        assert assert_multi_equals_lone(g, Q, ks, efs).fallback_queries == 3


@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("metric", METRICS)
def test_both_overflow_paths(metric, storage):
    Q = corpus(2000, 20)[1]
    ks, efs = mixed(len(Q), 13)
    with index(2000, 20, metric, storage) as g:
        g.set_heap_capacity(candidates=24)     # some walks outgrow 24 candidates and are answered by the spill launch, each with its ef
        st = assert_multi_equals_lone(g, Q, ks, efs)
        assert 0 < st.fallback_queries
        g.set_heap_capacity(results=8)         # ef_search 50 > 8: no results heap fits, every query goes straight to the spill launch
        st = assert_multi_equals_lone(g, Q, ks, efs)
        assert st.fallback_queries == len(Q)
        g.set_heap_capacity()
        assert assert_multi_equals_lone(g, Q, ks, efs).fallback_queries == 0


@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("n", [0, 1, 30])
def test_smallest_shapes(n, storage):
    """n = 30 is below every ef: the results heap is n + 1 entries; k above n leaves sentinels.  nq = 1.  kstride above every k."""
    d = 20
    Q = corpus(max(n, 1), d)[1]
    ks, efs = mixed(len(Q), 17)
    for metric in METRICS:
        with index(n, d, metric, storage) as g:
            assert_multi_equals_lone(g, Q, ks, efs)
            ids, sc, cnt = g.search_multi(Q, ks, efs)
            assert np.all(cnt <= np.minimum(ks, n)) and (n == 0 or np.all(cnt >= 1))
            assert_multi_equals_lone(g, Q[:1], ks[:1], efs[:1])                       # nq = 1
            assert_multi_equals_lone(g, Q[:7], np.minimum(ks[:7], 10), efs[:7], kstride=64)   # sentinels in [count, kstride)
            assert_multi_equals_lone(g, Q[:3], np.full(3, 5, np.uint32), np.zeros(3, np.uint32), kstride=5)  # the uniform launch


def test_golden_corpus_with_a_different_k_per_query():
    from neumann_amd import GpuHnsw, HNSWConfig
    z = np.load(GOLDEN)
    m, m0, efc, efs, metric = z["config"].tolist()
    K, Q = int(z["k"]), z["queries"]
    nq = len(Q)
    with GpuHnsw(Q.shape[1], HNSWConfig(m=m, m0=m0, ef_construction=efc, ef_search=efs, distance_metric=metric)) as g:
        g.insert(z["rows"])
        # every k from 1 to 64 once, ef = ef2 (120 >= every k): the walk of the frozen (k = 10, ef2) answers, cut at k
        ks = np.arange(1, nq + 1, dtype=np.uint32)
        assert efs >= 50 and int(z["ef2"]) >= nq
        ids, sc, cnt = g.search_multi(Q, ks, np.full(nq, int(z["ef2"]), np.uint32))
        for i in range(nq):
            c = min(int(ks[i]), K)
            assert cnt[i] >= c
            assert np.array_equal(ids[i, :c], z["ids_ef2"][i, :c]), i
            assert np.array_equal(sc[i, :c].view(np.uint32), z["scores_ef2"][i, :c].view(np.uint32)), i
        # ... and ef 0 with k 1 .. 50 (<= ef_search, so the walk is the frozen default one)
        ks = (np.arange(nq, dtype=np.uint32) % 50) + 1
        ids, sc, cnt = g.search_multi(Q, ks, None)
        for i in range(nq):
            c = min(int(ks[i]), K)
            assert np.array_equal(ids[i, :c], z["ids"][i, :c]), i
            assert np.array_equal(sc[i, :c].view(np.uint32), z["scores"][i, :c].view(np.uint32)), i


def test_bad_arguments_are_refused_and_nothing_is_written():
    import ctypes as C
    from neumann_amd import _capi
    Q = corpus(300, 5)[1][:4]
    with index(300, 5, 0, "dense") as g:
        for ks, status in (([3, 0, 3, 3], _capi.ERR_INVALID_TOP_K), ([3, 3, 3, 9], _capi.ERR_INVALID_ARGUMENT)):
            ids = np.full((4, 8), 7, np.uint64)
            sc = np.full((4, 8), 7, F)
            cnt = np.full(4, 7, np.uint32)
            kk = np.array(ks, np.uint32)
            rc = g._lib.nmn_hnsw_search_multi(g._h, C.c_void_p(Q.ctypes.data), 4, C.c_void_p(kk.ctypes.data), None, 8,
                                              C.c_void_p(ids.ctypes.data), C.c_void_p(sc.ctypes.data), C.c_void_p(cnt.ctypes.data), None)
            assert rc == status
            assert np.all(ids == 7) and np.all(sc == 7) and np.all(cnt == 7)
        with pytest.raises(_capi.NeumannGpuError) as e:
            g.search_multi(Q, [1, 2, 3, 4], kstride=3)
        assert e.value.status == _capi.ERR_INVALID_ARGUMENT
        assert g.search_multi(Q[:0], np.zeros(0, np.uint32), kstride=3)[0].shape == (0, 3)      # nq = 0: nothing enqueued


def test_host_walk_in_child_process(tmp_path):
    """NMN_HNSW_HOST_SEARCH=1 (the walk on the host, query by query) in a fresh child process: the same bits"""
    rows, Q = corpus(300, 33)
    ks, efs = mixed(len(Q), 19)
    np.savez(tmp_path / "in.npz", rows=rows, Q=Q, ks=ks, efs=efs)
    code = (
        "import sys, numpy as np\n"
        f"sys.path.insert(0, {ROOT!r})\n"
        "from neumann_amd import GpuHnsw, HNSWConfig\n"
        f"d = {str(tmp_path)!r}\n"
        "z = np.load(d + '/in.npz')\n"
        "for storage in ('dense', 'quantized'):\n"
        "    with GpuHnsw(z['rows'].shape[1], HNSWConfig().with_distance_metric(1), storage=storage) as g:\n"
        "        g.insert(z['rows'])\n"
        "        ids, sc, cnt, st = g.search_multi(z['Q'], z['ks'], z['efs'], kstride=256, with_stats=True)\n"
        "        assert st.sweep_launches == 0, st.sweep_launches\n"
        "        np.savez(d + f'/out_{storage}.npz', ids=ids, sc=sc, cnt=cnt, evals=st.rows_scanned)\n"
    )
    env = dict(os.environ, NMN_HNSW_HOST_SEARCH="1")
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    for storage in STORAGES:
        out = np.load(tmp_path / f"out_{storage}.npz")
        with index(300, 33, 1, storage) as g:
            ids, sc, cnt, st = g.search_multi(Q, ks, efs, kstride=256, with_stats=True)
            assert np.array_equal(ids, out["ids"]) and np.array_equal(cnt, out["cnt"])
            assert np.array_equal(sc.view(np.uint32), out["sc"].view(np.uint32))
            if storage == "quantized":   # (a dense handle's device walk counts its evaluations differently from the host walk)
                assert st.rows_scanned == int(out["evals"])
