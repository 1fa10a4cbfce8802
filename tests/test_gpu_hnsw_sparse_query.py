"""nmn_hnsw_search_sparse / GpuHnsw.search_sparse against tests/_hnsw_sparse_query_oracle.py: HNSWIndex::search_sparse_with_ef
walked on the GPU — ids exact, score BITS equal, counts equal, every query compared in full (docs/hnsw.md §13)."""
import functools
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

from tests import _hnsw_oracle as ho
from tests import _hnsw_q8_oracle as q8
from tests import _hnsw_sparse_query_oracle as so
from tests import _xmetric_oracle as xo

pytestmark = pytest.mark.gpu
F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "hnsw_small_sparse.npz")
METRICS = [ho.COSINE, ho.EUCLIDEAN, ho.DOT_PRODUCT]
STORAGES = ["dense", "quantized"]


def o_cfg(metric):
    return ho.HNSWConfig.high_speed().with_distance_metric(metric)


def g_cfg(metric):
    from neumann_amd import HNSWConfig
    return HNSWConfig.high_speed().with_distance_metric(metric)


@functools.lru_cache(maxsize=None)
def corpus(name):
    """name = kind:n:dim -> (rows, dense queries).  mix: half the rows have 60 % zeros, the others none; queries 80 % zeros.
    special: a quarter of the rows duplicates of earlier ones, a few zero rows."""
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


@functools.lru_cache(maxsize=None)
def oracle(name, storage, metric):
    return (q8.build if storage == "quantized" else ho.build)(corpus(name)[0], o_cfg(metric))


def gpu_index(name, storage, metric):
    from neumann_amd import GpuHnsw
    rows = corpus(name)[0]
    g = GpuHnsw(rows.shape[1], g_cfg(metric), storage=storage)
    g.insert(rows)
    return g


def assert_graph(g, o):
    assert len(g) == len(o)
    assert g.entry_point == o.entry_point and g.max_layer == o.max_layer
    assert g.levels().tolist() == o.levels
    for node in range(len(o)):
        for layer in range(o.levels[node] + 1):
            assert g.neighbors(node, layer).tolist() == o.neighbors[node][layer], (node, layer)


def assert_same(got, want):
    ig, sg, cg = got[:3]
    iw, sw, cw = want[:3]
    assert np.array_equal(cg, cw), (cg, cw)
    assert np.array_equal(ig, iw), np.argwhere(ig != iw)[:5]
    assert np.array_equal(np.ascontiguousarray(sg).view(np.uint32), np.ascontiguousarray(sw).view(np.uint32)), \
        np.argwhere(np.ascontiguousarray(sg).view(np.uint32) != np.ascontiguousarray(sw).view(np.uint32))[:5]


def want_sparse(o, dim, csr, k, ef):
    return so.padded_answers(o, so.queries_from_csr(dim, *csr), k, ef)


def expected_rows_scanned(o, storage, nq, evals):
    """the handle's convention for dense queries (docs/hnsw.md §9): a quantized handle reports the evaluations the reference makes; a
    dense handle carries the entry's distance from layer to layer, max_layer evaluations fewer per query"""
    return evals if storage == "quantized" or len(o) == 0 else evals - nq * o.max_layer


def check(g, o, storage, csr, k, ef, dim):
    want, evals = want_sparse(o, dim, csr, k, ef)
    ids, sc, cnt, st = g.search_sparse(*csr, k, ef, with_stats=True)
    assert_same((ids, sc, cnt), want)
    nq = len(csr[0]) - 1
    assert st.sweep == "graph" and st.rows_scanned == expected_rows_scanned(o, storage, nq, evals), (st.rows_scanned, evals)
    return (ids, sc, cnt), st


# ---- 1. the golden corpus ---------------------------------------------------------------------------------------------------------------
def test_golden_corpus():
    from neumann_amd import GpuHnsw, HNSWConfig
    rows, queries = xo.sparse_golden_corpus()
    o = xo.index_from_golden(GOLDEN)
    with GpuHnsw(rows.shape[1], HNSWConfig()) as g:
        g.insert(rows)
        assert_graph(g, o)
        csr = g.sparse_from_dense(queries)
        for a, b in zip(csr, so.csr_from_dense(queries)):
            assert a.dtype == b.dtype and np.array_equal(a.view(np.uint32) if a.dtype == F else a, b.view(np.uint32) if b.dtype == F else b)
        for ef in (50, 200):
            (ids, sc, cnt), st = check(g, o, "dense", csr, 10, ef, rows.shape[1])
            assert st.fallback_queries == 0
        (ids, sc, cnt), _ = check(g, o, "dense", csr, 10, 50, rows.shape[1])
        _, dsc, _ = g.search(queries, 10, 50)
        differ = int((sc.view(np.uint32) != dsc.view(np.uint32)).any(axis=1).sum())
        print(f"score bits differ from the dense walk of the same queries for {differ} of {len(queries)}")
        assert differ >= 32                      # a densifying shortcut fails here


# ---- 2. metrics x storages, and the shapes of sparse_distance -----------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [20, 33])
@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("metric", METRICS)
def test_metrics_and_storages(metric, storage, dim):
    name = f"mix:300:{dim}"
    o = oracle(name, storage, metric)
    Q = corpus(name)[1]
    with gpu_index(name, storage, metric) as g:
        assert_graph(g, o)
        csr = g.sparse_from_dense(Q)
        check(g, o, storage, csr, 10, 50, dim)
        check(g, o, storage, csr, 305, None, dim)            # k > n: ef = k, every node the walk reaches
        if metric == ho.EUCLIDEAN or (storage == "quantized" and metric == ho.DOT_PRODUCT):
            assert_same(g.search_sparse(*csr, 10, 50), g.search(Q, 10, 50))   # bit for bit the dense walk of to_dense(Q)


@pytest.mark.parametrize("dim", [5, 8, 128, 771])
def test_dimensions_cosine_dense(dim):
    """an odd entry count below one pass of four pairs, exactly one, many"""
    name = f"mix:200:{dim}"
    o = oracle(name, "dense", ho.COSINE)
    Q = corpus(name)[1].copy()
    Q[4] = corpus(name)[0][3]
    Q[4][Q[4] == 0] = F(0.5)                                  # every position stored
    with gpu_index(name, "dense", ho.COSINE) as g:
        assert_graph(g, o)
        check(g, o, "dense", g.sparse_from_dense(Q), 10, 50, dim)


# ---- 3. special queries, in one call --------------------------------------------------------------------------------------------------------
def special_csr(dim, rows):
    full = rows[5].copy()
    full[full == 0] = F(-1.25)
    parts = [
        ([], []),                                                         # no stored entry
        ([dim - 1], [F(2.5)]),                                            # one entry
        (list(range(dim)), full.tolist()),                                # every position stored
        ([7, 2, 9, 2, 0, 4, 2], [1.5, -3.0, 0.0, 4.0, -0.0, 0.25, -8.0]),  # unsorted, zeros of both signs, position 2 three times
        ([3, 1], [0.0, -0.0]),                                            # only zeros: no stored entry either
    ]
    indptr = np.cumsum([0] + [len(p) for p, _ in parts]).astype(np.uint64)
    pos = np.array([x for p, _ in parts for x in p], dtype=np.uint32)
    val = np.array([x for _, v in parts for x in v], dtype=F)
    return indptr, pos, val


@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("metric", METRICS)
def test_special_queries(metric, storage):
    name = "special:240:12"
    o = oracle(name, storage, metric)
    rows = corpus(name)[0]
    csr = special_csr(12, rows)
    with gpu_index(name, storage, metric) as g:
        assert_graph(g, o)
        (ids, sc, cnt), _ = check(g, o, storage, csr, 10, 50, 12)
        check(g, o, storage, csr, 245, None, 12)
        if metric == ho.COSINE:
            assert np.all(sc[0] == 0.0) and np.all(sc[4] == 0.0)          # every distance 1.0: the tie rules decided the ids
        if metric == ho.DOT_PRODUCT and storage == "dense":
            assert np.all(sc[0] == 0.0) and np.all(np.signbit(sc[0]))     # dot -0.0, distance +0.0, similarity -0.0


# ---- 4. both overflow paths ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("storage,metric", [("dense", ho.COSINE), ("dense", ho.DOT_PRODUCT), ("quantized", ho.COSINE)])
def test_overflow_paths(storage, metric):
    name = "mix:300:20"
    o = oracle(name, storage, metric)
    Q = corpus(name)[1]
    with gpu_index(name, storage, metric) as g:
        csr = g.sparse_from_dense(Q)
        g.set_heap_capacity(results=0, candidates=16)
        _, st = check(g, o, storage, csr, 10, 50, 20)
        assert st.fallback_queries > 0
        g.set_heap_capacity(results=16)
        _, st = check(g, o, storage, csr, 10, 50, 20)
        assert st.fallback_queries == len(Q)
        g.set_heap_capacity()
        _, st = check(g, o, storage, csr, 10, 50, 20)
        assert st.fallback_queries == 0


# ---- 5. the host walk ---------------------------------------------------------------------------------------------------------------------
def test_host_search_env_in_child_process(tmp_path):
    """NMN_HNSW_HOST_SEARCH=1 in a fresh child process: the sparse host walk, the same bits"""
    name = "mix:300:20"
    rows, Q = corpus(name)
    np.save(tmp_path / "rows.npy", rows)
    np.save(tmp_path / "q.npy", Q)
    code = (
        "import sys, numpy as np\n"
        f"sys.path.insert(0, {ROOT!r})\n"
        "from neumann_amd import GpuHnsw, HNSWConfig\n"
        f"d = {str(tmp_path)!r}\n"
        "rows, Q = np.load(d + '/rows.npy'), np.load(d + '/q.npy')\n"
        "for storage in ('dense', 'quantized'):\n"
        "    for metric in (0, 1, 2):\n"
        "        with GpuHnsw(rows.shape[1], HNSWConfig.high_speed().with_distance_metric(metric), storage=storage) as g:\n"
        "            g.insert(rows)\n"
        "            ids, sc, cnt, st = g.search_sparse(*g.sparse_from_dense(Q), 10, 50, with_stats=True)\n"
        "            assert st.sweep_launches == 0, st.sweep_launches\n"
        "            np.savez(d + f'/out_{storage}_{metric}.npz', ids=ids, sc=sc, cnt=cnt, evals=st.rows_scanned)\n"
    )
    env = dict(os.environ, NMN_HNSW_HOST_SEARCH="1")
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    csr = so.csr_from_dense(Q)
    for storage in STORAGES:
        for metric in METRICS:
            o = oracle(name, storage, metric)
            out = np.load(tmp_path / f"out_{storage}_{metric}.npz")
            want, evals = want_sparse(o, 20, csr, 10, 50)
            assert_same((out["ids"], out["sc"], out["cnt"]), want)
            assert int(out["evals"]) == evals     # the host walk counts what the reference evaluates, on either handle


# ---- 6. more stored entries than a wave keeps in LDS -------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", [ho.COSINE, ho.DOT_PRODUCT])
def test_more_than_4096_entries(metric):
    rng = np.random.default_rng(8192)
    dim, n = 8192, 40
    rows = rng.standard_normal((n, dim)).astype(F)
    rows[rng.random(rows.shape) < 0.5] = 0.0
    o = ho.build(rows, o_cfg(metric))
    big = np.zeros(dim, dtype=F)
    at = rng.choice(dim, 5000, replace=False)
    big[at] = rng.standard_normal(5000).astype(F)
    small = np.zeros(dim, dtype=F)
    small[rng.choice(dim, 10, replace=False)] = F(1.5)
    limit = np.zeros(dim, dtype=F)
    limit[rng.choice(dim, 4096, replace=False)] = F(-0.75)     # exactly what fits: walked on the device
    from neumann_amd import GpuHnsw
    with GpuHnsw(dim, g_cfg(metric)) as g:
        g.insert(rows)
        assert_graph(g, o)
        csr = g.sparse_from_dense(np.stack([big, small, limit]))
        assert np.diff(csr[0].astype(np.int64)).tolist() == [5000, 10, 4096]
        want, _ = want_sparse(o, dim, csr, 10, 50)
        assert_same(g.search_sparse(*csr, 10, 50), want)


# ---- 7. refusals, with nothing written; empty and one-row indexes ---------------------------------------------------------------------------
def test_refusals_and_edges():
    from neumann_amd import GpuHnsw, NeumannGpuError, _capi
    import ctypes as C
    with GpuHnsw(6, g_cfg(ho.COSINE)) as g:
        ids, sc, cnt, st = g.search_sparse([0, 1, 1], [2], [1.0], 3, with_stats=True)       # n = 0
        assert cnt.tolist() == [0, 0] and np.all(ids == np.uint64(0xFFFFFFFFFFFFFFFF)) and np.all(np.isneginf(sc))
        assert st.rows_scanned == 0
        g.insert(np.arange(6, dtype=F)[None, :])                                             # n = 1
        o = ho.build(np.arange(6, dtype=F)[None, :], o_cfg(ho.COSINE))
        check(g, o, "dense", (np.array([0, 1, 1], np.uint64), np.array([2], np.uint32), np.array([1.0], F)), 3, None, 6)
        g.insert(np.eye(6, dtype=F))
        lib, h = g._lib, g._h

        def raw(indptr, pos, val, nq, k):
            ip, p, v = np.asarray(indptr, np.uint64), np.asarray(pos, np.uint32), np.asarray(val, F)
            ids = np.full((max(nq, 1), max(k, 1)), 12345, dtype=np.uint64)
            sc = np.full((max(nq, 1), max(k, 1)), 7.0, dtype=F)
            cnt = np.full(max(nq, 1), 99, dtype=np.uint32)
            st = lib.nmn_hnsw_search_sparse(h, C.c_void_p(ip.ctypes.data), C.c_void_p(p.ctypes.data), C.c_void_p(v.ctypes.data), nq, k, 0,
                                            C.c_void_p(ids.ctypes.data), C.c_void_p(sc.ctypes.data), C.c_void_p(cnt.ctypes.data), None)
            untouched = bool(np.all(ids == 12345) and np.all(sc == 7.0) and np.all(cnt == 99))
            return st, untouched, lib.nmn_last_error().decode(errors="replace")

        st, untouched, _ = raw([0, 1], [0], [1.0], 1, 0)
        assert st == _capi.ERR_INVALID_TOP_K and untouched
        st, untouched, text = raw([0, 1, 2], [0, 6], [1.0, 1.0], 2, 3)                       # a position == dim, in the SECOND query
        assert st == _capi.ERR_INVALID_ARGUMENT and untouched
        assert "index 6" in text and "dimension 6" in text
        st, untouched, _ = raw([0, 2, 1], [0, 1], [1.0, 1.0], 2, 3)
        assert st == _capi.ERR_INVALID_ARGUMENT and untouched                                # a decreasing indptr
        st, untouched, _ = raw([0], [], [], 0, 3)                                            # nq == 0: nothing enqueued, nothing written
        assert st == 0 and untouched
        with pytest.raises(NeumannGpuError) as e:
            g.search_sparse([0, 1], [6], [0.0], 3)                                           # checked before the zero is dropped
        assert e.value.status == _capi.ERR_INVALID_ARGUMENT
        ids, sc, cnt = g.search_sparse([0], [], [], 3)
        assert ids.shape == (0, 3) and cnt.size == 0


# ---- 8. concurrency ----------------------------------------------------------------------------------------------------------------------
def test_dense_and_sparse_callers_on_one_handle():
    name = "mix:300:20"
    rows, Q = corpus(name)
    with gpu_index(name, "dense", ho.COSINE) as g:
        csr = g.sparse_from_dense(Q)
        alone_sparse = g.search_sparse(*csr, 10, 50)
        alone_dense = g.search(Q, 10, 50)
        out, errs = [None] * 8, []

        def run(t):
            try:
                for _ in range(5):
                    out[t] = g.search_sparse(*csr, 10, 50) if t % 2 else g.search(Q, 10, 50)
            except Exception as e:  # noqa: BLE001
                errs.append(e)

        threads = [threading.Thread(target=run, args=(t,)) for t in range(8)]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
        assert not errs, errs
        for t in range(8):
            assert_same(out[t], alone_sparse if t % 2 else alone_dense)
