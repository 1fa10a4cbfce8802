"""nmn_hnsw_search_metric_multi (GpuHnsw.search_metric_multi, docs/hnsw.md §12): one call that carries a top_k and a metric per
query.  The answer for query i must be bit for bit what nmn_hnsw_search_metric(q_i, 1, top_k[i], &metrics[i]) returns alone — ids,
score bits, counts, sentinels and the stats — for all nine metrics in one call (every chain family, two kinds with different
closings in a family), on both sides of the LDS limit, through both overflow paths and on both sides of the sort threshold.  The lone
call is the uniform chain tests/test_gpu_xmetric.py holds to the oracle; the sparse golden corpus ties the mixed call to the oracle
directly.  Angular / Geodesic are the same code in both forms, so the same bits here; against the oracle they keep §8's one-ulp rule."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import _xmetric_oracle as xo
from tests.test_gpu_hnsw_multi import corpus

pytestmark = pytest.mark.gpu
F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U64_MAX = np.uint64(0xFFFFFFFFFFFFFFFF)
TOPS = (1, 5, 6, 10, 64, 200)            # c = 10, 10, 12, 20, 128, 400: 400 is more than one workgroup's 256 pairs
ACOS = (xo.ANGULAR, xo.GEODESIC)
SIM_TOL = 2.0 ** -22                     # docs/hnsw.md §8: one ulp of acos, divided by pi, two roundings


def nine():
    from neumann_amd import ExtendedDistanceMetric as M, GeometricConfig
    return [M(k) for k in range(8)] + [M.Composite(GeometricConfig(0.2, 0.7, 0.1))]


def mixed(nq, seed):
    """a top_k and a metric per query: every value of TOPS and all nine metrics present, in no particular pairing"""
    rng = np.random.default_rng(seed)
    tops = np.array([TOPS[i % len(TOPS)] for i in range(nq)], np.uint32)
    rng.shuffle(tops)
    m9 = nine()
    return tops, [m9[(i * 4) % 9] for i in range(nq)]


def index(n, d, preset="default"):
    from neumann_amd import GpuHnsw, HNSWConfig
    g = GpuHnsw(d, getattr(HNSWConfig, preset)())
    if n:
        g.insert(corpus(n, d)[0])
    return g


def bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


def assert_multi_equals_lone(g, Q, tops, metrics, kstride=None):
    """one search_metric_multi call against one lone search_metric call per query; returns the multi call's stats"""
    ids, sc, cnt, st = g.search_metric_multi(Q, tops, metrics, kstride=kstride, with_stats=True)
    kstride = int(max(tops)) if kstride is None else kstride
    assert ids.shape == sc.shape == (len(Q), kstride)
    evals = spilled = rescored = 0
    kinds, launches = set(), set()
    for i in range(len(Q)):
        k = int(tops[i])
        li, ls, lc, lst = g.search_metric(Q[i], k, metrics[i], with_stats=True)
        assert cnt[i] == lc[0], (i, k, cnt[i], lc[0])
        assert np.array_equal(ids[i, :k], li[0]), (i, k, metrics[i])
        assert np.array_equal(bits(sc[i, :k]), bits(ls[0])), (i, k, metrics[i])
        assert np.all(ids[i, cnt[i]:] == U64_MAX) and np.all(np.isneginf(sc[i, cnt[i]:])), (i, k)
        evals += lst.rows_scanned
        spilled += lst.fallback_queries
        rescored = max(rescored, lst.candidates_rescored)
        kinds.add(lst.sweep_kind)
        launches.add(lst.sweep_launches)
    assert st.rows_scanned == evals, (st.rows_scanned, evals)
    assert st.fallback_queries == spilled, (st.fallback_queries, spilled)
    assert st.candidates_rescored == rescored, (st.candidates_rescored, rescored)
    assert kinds == {st.sweep_kind} and launches == {st.sweep_launches}
    return st


@pytest.mark.parametrize("n,d", [(2000, 20), (300, 5), (300, 33)])
def test_all_nine_metrics_and_every_top_k_in_one_call(n, d):
    Q = corpus(n, d)[1]
    tops, metrics = mixed(len(Q), 7)
    assert {m.kind for m in metrics} == set(range(9)) and set(tops.tolist()) == set(TOPS)
    with index(n, d) as g:
        st = assert_multi_equals_lone(g, Q, tops, metrics, kstride=256)      # kstride above the largest top_k
        assert st.fallback_queries == 0
        assert st.candidates_rescored <= min(400, n)                         # at n = 300, c = 400 is capped to len
        assert n < 2000 or st.candidates_rescored > 256                      # ... and at 2 000 more than one workgroup's pairs
        assert_multi_equals_lone(g, Q, tops, metrics)                        # kstride = max(top_k)
        one = [metrics[3]] * len(Q)                                          # one metric, many top_k; one top_k, many metrics
        assert_multi_equals_lone(g, Q, tops, one, kstride=201)
        assert_multi_equals_lone(g, Q[:18], np.full(18, 10, np.uint32), nine() * 2, kstride=10)


def test_golden_sparse_corpus_against_the_oracle():
    """mixed metrics and top_k over tests/golden/hnsw_small_sparse.npz, against the oracle's walk and its metrics directly"""
    from tests.test_gpu_xmetric import g_metric, walk_corpus, walk_gpu, walk_reference
    rows, Q = walk_corpus("sparse")
    g = walk_gpu("sparse")
    o_metrics = [xo.Metric(k) for k in range(8)] + [xo.Metric(xo.COMPOSITE, xo.GeometricConfig.default())]
    tops_of = (1, 5, 10)
    tops = np.array([tops_of[i % 3] for i in range(len(Q))], np.uint32)
    om = [o_metrics[(i * 4 + i // 9) % 9] for i in range(len(Q))]
    assert {m.kind for m in om} == set(range(9))
    ids, sc, cnt = g.search_metric_multi(Q, tops, [g_metric(m) for m in om], kstride=16)
    for i in range(len(Q)):
        k = int(tops[i])
        w_ids, w_sc, w_cnt, _ = walk_reference("sparse", om[i], k)
        assert cnt[i] == w_cnt[i], i
        assert np.all(ids[i, cnt[i]:] == U64_MAX) and np.all(np.isneginf(sc[i, cnt[i]:])), i
        if om[i].kind in ACOS:   # §8: ids where one ulp of acos cannot reorder (test_gpu_xmetric states when), scores within 2^-22
            assert np.array_equal(ids[i, :k], w_ids[i]), (i, om[i])
            used = w_ids[i] != U64_MAX
            diff = np.abs(sc[i, :k][used].astype(np.float64) - w_sc[i][used].astype(np.float64))
            print(f"query {i} {xo.NAMES[om[i].kind]} top_k={k}: similarity max |diff| {diff.max():.3e}")
            assert diff.max() <= SIM_TOL, (i, om[i])
        else:
            assert np.array_equal(ids[i, :k], w_ids[i]), (i, om[i])
            assert np.array_equal(bits(sc[i, :k]), bits(w_sc[i])), (i, om[i])


@pytest.mark.parametrize("n", [0, 1, 30])
def test_smallest_shapes(n):
    d = 20
    Q = corpus(max(n, 1), d)[1]
    m9 = nine()
    tops = np.array([(1, 20, 40)[i % 3] for i in range(len(Q))], np.uint32)
    metrics = [m9[(i * 4) % 9] for i in range(len(Q))]
    with index(n, d) as g:
        assert_multi_equals_lone(g, Q, tops, metrics)
        ids, sc, cnt = g.search_metric_multi(Q, tops, metrics, kstride=64)
        assert np.all(cnt <= np.minimum(tops, n)) and (n == 0 or np.all(cnt >= 1))
        assert_multi_equals_lone(g, Q[:1], tops[:1], metrics[:1])                        # nq = 1, the uniform chain
        assert_multi_equals_lone(g, Q[:1], tops[:1], metrics[:1], kstride=7)             # nq = 1, rows longer than top_k
        assert_multi_equals_lone(g, Q[:7], tops[:7], metrics[:7], kstride=64)


def test_a_call_that_straddles_the_lds_limit():
    """one query at top_k 600: c = 1 200 candidates, a results heap of 1 201 entries that no wave keeps in LDS, so it goes straight
    to the spill launch while the others start in LDS"""
    Q = corpus(2000, 20)[1]
    tops, metrics = mixed(len(Q), 11)
    tops[17] = 600
    with index(2000, 20) as g:
        st = assert_multi_equals_lone(g, Q, tops, metrics, kstride=600)
        assert st.fallback_queries == 1
        tops[[0, 39]] = 600, 520                                    # the first and the last of the call too
        assert assert_multi_equals_lone(g, Q, tops, metrics, kstride=640).fallback_queries == 3


def test_both_overflow_paths():
    Q = corpus(2000, 20)[1]
    tops, metrics = mixed(len(Q), 13)
    with index(2000, 20) as g:
        g.set_heap_capacity(candidates=24)     # some walks outgrow 24 candidates and are answered by the spill launch
        st = assert_multi_equals_lone(g, Q, tops, metrics)
        assert 0 < st.fallback_queries
        g.set_heap_capacity(results=8)         # ef_search 50 > 8: no results heap fits, every query goes straight to the spill launch
        st = assert_multi_equals_lone(g, Q, tops, metrics)
        assert st.fallback_queries == len(Q)
        g.set_heap_capacity()
        assert assert_multi_equals_lone(g, Q, tops, metrics).fallback_queries == 0


def _child(tmp_path, env, body):
    code = (
        "import sys, numpy as np\n"
        f"sys.path.insert(0, {ROOT!r})\n"
        "from neumann_amd import GpuHnsw, HNSWConfig, ExtendedDistanceMetric as M, GeometricConfig\n"
        f"d = {str(tmp_path)!r}\n"
        "z = np.load(d + '/in.npz')\n"
        "m9 = [M(k) for k in range(8)] + [M.Composite(GeometricConfig(0.2, 0.7, 0.1))]\n"
        "metrics = [m9[k] for k in z['kinds']]\n"
        "with GpuHnsw(z['rows'].shape[1], HNSWConfig()) as g:\n"
        "    g.insert(z['rows'])\n"
        "    ids, sc, cnt, st = g.search_metric_multi(z['Q'], z['tops'], metrics, kstride=256, with_stats=True)\n"
        + body +
        "    np.savez(d + '/out.npz', ids=ids, sc=sc, cnt=cnt)\n"
    )
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, **env), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return np.load(tmp_path / "out.npz")


def _child_case(tmp_path, n, d, seed):
    rows, Q = corpus(n, d)
    tops, metrics = mixed(len(Q), seed)
    np.savez(tmp_path / "in.npz", rows=rows, Q=Q, tops=tops, kinds=np.array([m.kind for m in metrics]))
    with index(n, d) as g:
        want = g.search_metric_multi(Q, tops, metrics, kstride=256)
    return tops, want


def test_both_sides_of_the_sort_threshold_in_child_process(tmp_path):
    """NMN_XMETRIC_SORT_FROM=16 in a fresh child process: the queries with c = 10 and 12 are ranked, those with c = 20, 128 and 400
    go, each alone, through the large-k sort — one call holds both, and its answers equal the default threshold's, where the rank
    count orders every one"""
    tops, want = _child_case(tmp_path, 2000, 20, 23)
    assert (np.maximum(2 * tops, 10) <= 16).any() and (np.maximum(2 * tops, 10) >= 20).any()
    out = _child(tmp_path, {"NMN_XMETRIC_SORT_FROM": "16"}, "")
    assert np.array_equal(out["ids"], want[0]) and np.array_equal(out["cnt"], want[2])
    assert np.array_equal(bits(out["sc"]), bits(want[1]))


def test_host_walk_in_child_process(tmp_path):
    """NMN_HNSW_HOST_SEARCH=1 (the walk on the host, the re-rank on the device) in a fresh child process: the same bits"""
    tops, want = _child_case(tmp_path, 300, 33, 19)
    out = _child(tmp_path, {"NMN_HNSW_HOST_SEARCH": "1"}, "    assert st.sweep_launches == 0, st.sweep_launches\n")
    assert np.array_equal(out["ids"], want[0]) and np.array_equal(out["cnt"], want[2])
    assert np.array_equal(bits(out["sc"]), bits(want[1]))


def test_bad_arguments_are_refused_and_nothing_is_written():
    import ctypes as C
    from neumann_amd import GpuHnsw, HNSWConfig, _capi
    rows, Q = corpus(300, 5)
    Q = Q[:4]

    def call(g, tops, kinds):
        ids = np.full((4, 8), 7, np.uint64)
        sc = np.full((4, 8), 7, F)
        cnt = np.full(4, 7, np.uint32)
        kk = np.array(tops, np.uint32)
        mm = (_capi.XMetric * 4)(*[_capi.XMetric(kind=k, cosine_weight=0.5, structural_weight=0.3, magnitude_weight=0.2) for k in kinds])
        rc = g._lib.nmn_hnsw_search_metric_multi(g._h, C.c_void_p(Q.ctypes.data), 4, C.c_void_p(kk.ctypes.data), C.cast(mm, C.c_void_p), 8,
                                                 C.c_void_p(ids.ctypes.data), C.c_void_p(sc.ctypes.data), C.c_void_p(cnt.ctypes.data), None)
        assert np.all(ids == 7) and np.all(sc == 7) and np.all(cnt == 7)
        return rc

    with index(300, 5) as g:
        assert call(g, [3, 0, 3, 3], [0, 1, 2, 3]) == _capi.ERR_INVALID_TOP_K
        assert call(g, [3, 3, 3, 9], [0, 1, 2, 3]) == _capi.ERR_INVALID_ARGUMENT
        assert call(g, [3, 3, 3, 3], [0, 1, 2, 9]) == _capi.ERR_CONFIGURATION         # an unknown kind at the last query
        assert call(g, [3, 3, 3, 3], [-1, 1, 2, 3]) == _capi.ERR_CONFIGURATION
        assert g.search_metric_multi(Q[:0], np.zeros(0, np.uint32), [], kstride=3)[0].shape == (0, 3)   # nq = 0: nothing enqueued
    with GpuHnsw(5, HNSWConfig(), storage="quantized") as g:
        g.insert(rows)
        assert call(g, [3, 3, 3, 3], [0, 1, 2, 3]) == _capi.ERR_CONFIGURATION         # a quantized handle keeps no f32 rows
