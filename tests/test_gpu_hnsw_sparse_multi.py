"""nmn_hnsw_search_sparse_multi / GpuHnsw.search_sparse_multi (docs/hnsw.md §14): sparse queries with a k and an ef each, in one
launch that carries a query kind per query.  Row i must be the oracle's answer (tests/_hnsw_sparse_query_oracle.py) AND what
search_sparse of query i alone returns — ids exact, score BITS equal, counts equal — and the stats the sums of those lone calls'."""
import ctypes as C
import functools
import os

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
NONE_ID = np.uint64(0xFFFFFFFFFFFFFFFF)


def o_cfg(metric):
    return ho.HNSWConfig.high_speed().with_distance_metric(metric)


def g_cfg(metric):
    from neumann_amd import HNSWConfig
    return HNSWConfig.high_speed().with_distance_metric(metric)


@functools.lru_cache(maxsize=None)
def corpus(name):
    """the generator of test_gpu_hnsw_sparse_query.py.  name = kind:n:dim -> (rows, dense queries).  mix: half the rows have 60 %
    zeros, the others none; queries 80 % zeros.  special: a quarter of the rows duplicates of earlier ones, a few zero rows."""
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


def draw_k_ef(nq, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(1, 13, nq).astype(np.uint32), rng.choice(np.array([0, 5, 50, 200], np.uint32), nq)


def one(csr, i):
    """query i of a CSR as a CSR of its own"""
    a, b = int(csr[0][i]), int(csr[0][i + 1])
    return np.array([0, b - a], np.uint64), csr[1][a:b], csr[2][a:b]


def bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


_ORACLE_ROWS = {}


def oracle_rows(key, o, dim, csr, ks, efs):
    """per query: ([(id, similarity)], evaluations) from the oracle, computed once per (corpus, handle, k / ef draw)"""
    if key not in _ORACLE_ROWS:
        out = []
        for sq, k, ef in zip(so.queries_from_csr(dim, *csr), ks, efs):
            ev = []
            res = so.search_sparse_with_ef(o, sq, int(k), int(ef) if ef else o.config.ef_search, ev)
            out.append((res, int(sum(ev))))
        _ORACLE_ROWS[key] = out
    return _ORACLE_ROWS[key]


def rows_scanned_of(o, storage, evals):
    """the handle's convention (docs/hnsw.md §9): a dense handle reports max_layer evaluations fewer per query than the reference makes"""
    return evals if storage == "quantized" or len(o) == 0 else evals - o.max_layer


def check_multi(g, o, storage, dim, csr, ks, efs, kstride, key, host_walked=()):
    """row i == the oracle == search_sparse of query i alone; stats == the sums of the lone calls'.  host_walked: the queries the
    host walk answers, which counts what the reference evaluates on either handle"""
    nq = len(csr[0]) - 1
    ids, sc, cnt, st = g.search_sparse_multi(*csr, ks, efs, kstride=kstride, with_stats=True)
    assert ids.shape == (nq, kstride) and sc.shape == (nq, kstride)
    want = oracle_rows(key, o, dim, csr, ks, efs)
    rows = bytes_ = fallback = 0
    for i in range(nq):
        k = int(ks[i])
        res, evals = want[i]
        assert cnt[i] == len(res), (i, cnt[i], len(res))
        assert ids[i, :len(res)].tolist() == [r[0] for r in res], i
        assert bits(sc[i, :len(res)]).tolist() == bits(np.array([r[1] for r in res], F)).tolist(), i
        assert np.all(ids[i, len(res):] == NONE_ID) and np.all(np.isneginf(sc[i, len(res):])), i
        lids, lsc, lcnt, lst = g.search_sparse(*one(csr, i), k, int(efs[i]) or None, with_stats=True)
        assert lcnt[0] == cnt[i] and np.array_equal(lids[0], ids[i, :k]) and np.array_equal(bits(lsc[0]), bits(sc[i, :k])), i
        assert lst.rows_scanned == (evals if i in host_walked else rows_scanned_of(o, storage, evals)), (i, lst.rows_scanned, evals)
        rows += lst.rows_scanned
        bytes_ += lst.bytes_scanned
        fallback += lst.fallback_queries
        assert lst.sweep_launches == st.sweep_launches and lst.sweep == st.sweep
    assert (st.rows_scanned, st.bytes_scanned, st.fallback_queries) == (rows, bytes_, fallback)
    return st


# ---- 1. metrics x storages, a k and an ef per query ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [20, 33])
@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("metric", METRICS)
def test_metrics_and_storages(metric, storage, dim):
    name = f"mix:300:{dim}"
    o = oracle(name, storage, metric)
    Q = corpus(name)[1]
    ks, efs = draw_k_ef(len(Q), 1000 + dim)
    assert len(set(ks.tolist())) > 3 and set(efs.tolist()) == {0, 5, 50, 200}
    with gpu_index(name, storage, metric) as g:
        csr = g.sparse_from_dense(Q)
        for kstride in (12, 16):
            st = check_multi(g, o, storage, dim, csr, ks, efs, kstride, (name, storage, metric))
            assert st.sweep == "graph" and st.fallback_queries == 0
        if metric == ho.EUCLIDEAN or (storage == "quantized" and metric == ho.DOT_PRODUCT):
            a, b = g.search_sparse_multi(*csr, ks, efs, kstride=12), g.search_multi(Q, ks, efs, kstride=12)
            assert np.array_equal(a[0], b[0]) and np.array_equal(bits(a[1]), bits(b[1])) and np.array_equal(a[2], b[2])


def test_golden_corpus():
    from neumann_amd import GpuHnsw, HNSWConfig
    rows, queries = xo.sparse_golden_corpus()
    o = xo.index_from_golden(GOLDEN)
    queries = queries[:24]
    ks, efs = draw_k_ef(len(queries), 77)
    with GpuHnsw(rows.shape[1], HNSWConfig()) as g:
        g.insert(rows)
        check_multi(g, o, "dense", rows.shape[1], g.sparse_from_dense(queries), ks, efs, 12, "golden")


# ---- 2. special queries, in one call --------------------------------------------------------------------------------------------------------
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
    csr = special_csr(12, corpus(name)[0])
    ks, efs = np.array([10, 3, 12, 7, 1], np.uint32), np.array([50, 0, 5, 200, 50], np.uint32)
    with gpu_index(name, storage, metric) as g:
        check_multi(g, o, storage, 12, csr, ks, efs, 12, (name, storage, metric))
        ids, sc, cnt = g.search_sparse_multi(*csr, ks, efs)
        if metric == ho.COSINE:
            assert np.all(sc[0, :10] == 0.0) and np.all(sc[4, :1] == 0.0)   # every distance 1.0: the tie rules decided the ids
        if metric == ho.DOT_PRODUCT and storage == "dense":
            assert np.all(sc[0, :10] == 0.0) and np.all(np.signbit(sc[0, :10]))  # dot -0.0, distance +0.0, similarity -0.0


# ---- 3. both overflow paths -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("storage,metric", [("dense", ho.COSINE), ("dense", ho.DOT_PRODUCT), ("quantized", ho.COSINE)])
def test_overflow_paths(storage, metric):
    name = "mix:300:20"
    o = oracle(name, storage, metric)
    Q = corpus(name)[1]
    ks, efs = draw_k_ef(len(Q), 1020)
    key = (name, storage, metric)
    with gpu_index(name, storage, metric) as g:
        csr = g.sparse_from_dense(Q)
        g.set_heap_capacity(results=0, candidates=16)
        st = check_multi(g, o, storage, 20, csr, ks, efs, 12, key)       # (fallback_queries == the lone calls' sum, in check_multi)
        assert 0 < st.fallback_queries
        g.set_heap_capacity(results=4)
        st = check_multi(g, o, storage, 20, csr, ks, efs, 12, key)
        assert st.fallback_queries == len(Q)                               # every ef is 5 or more: no results heap fits four entries
        g.set_heap_capacity()
        st = check_multi(g, o, storage, 20, csr, ks, efs, 12, key)
        assert st.fallback_queries == 0


# ---- 4. refusals, with nothing written; empty and one-row indexes ---------------------------------------------------------------------------
def test_refusals_and_edges():
    from neumann_amd import GpuHnsw, NeumannGpuError, _capi
    with GpuHnsw(6, g_cfg(ho.COSINE)) as g:
        ids, sc, cnt, st = g.search_sparse_multi([0, 1, 1], [2], [1.0], [3, 1], with_stats=True)   # n = 0
        assert ids.shape == (2, 3) and cnt.tolist() == [0, 0] and np.all(ids == NONE_ID) and np.all(np.isneginf(sc))
        assert st.rows_scanned == 0
        one_row = np.arange(6, dtype=F)[None, :]
        g.insert(one_row)                                                                          # n = 1
        o = ho.build(one_row, o_cfg(ho.COSINE))
        csr = (np.array([0, 1, 1, 3], np.uint64), np.array([2, 5, 0], np.uint32), np.array([1.0, -2.0, 0.5], F))
        check_multi(g, o, "dense", 6, csr, np.array([3, 1, 2], np.uint32), np.array([0, 5, 50], np.uint32), 4, "n1")
        g.insert(np.eye(6, dtype=F))
        lib, h = g._lib, g._h

        def raw(indptr, pos, val, nq, k, kstride, ef=None):
            ip, p, v = np.asarray(indptr, np.uint64), np.asarray(pos, np.uint32), np.asarray(val, F)
            kk = np.asarray(k, np.uint32)
            ee = None if ef is None else np.asarray(ef, np.uint32)
            ids = np.full((max(nq, 1), max(kstride, 1)), 12345, dtype=np.uint64)
            sc = np.full((max(nq, 1), max(kstride, 1)), 7.0, dtype=F)
            cnt = np.full(max(nq, 1), 99, dtype=np.uint32)
            st = lib.nmn_hnsw_search_sparse_multi(h, C.c_void_p(ip.ctypes.data), C.c_void_p(p.ctypes.data), C.c_void_p(v.ctypes.data), nq,
                                                  C.c_void_p(kk.ctypes.data), None if ee is None else C.c_void_p(ee.ctypes.data), kstride,
                                                  C.c_void_p(ids.ctypes.data), C.c_void_p(sc.ctypes.data), C.c_void_p(cnt.ctypes.data), None)
            untouched = bool(np.all(ids == 12345) and np.all(sc == 7.0) and np.all(cnt == 99))
            return st, untouched, lib.nmn_last_error().decode(errors="replace")

        st, untouched, _ = raw([0, 1, 2], [0, 1], [1.0, 1.0], 2, [3, 0], 4)
        assert st == _capi.ERR_INVALID_TOP_K and untouched                                   # k[1] == 0
        st, untouched, text = raw([0, 1, 2], [0, 1], [1.0, 1.0], 2, [3, 5], 4)
        assert st == _capi.ERR_INVALID_ARGUMENT and untouched and "kstride" in text          # k[1] above kstride
        st, untouched, _ = raw([0, 1], [0], [1.0], 1, [1], 0)
        assert st == _capi.ERR_INVALID_TOP_K and untouched                                   # kstride == 0
        st, untouched, text = raw([0, 1, 2], [0, 6], [1.0, 1.0], 2, [3, 2], 4)               # a position == dim, in the SECOND query
        assert st == _capi.ERR_INVALID_ARGUMENT and untouched
        assert "index 6" in text and "dimension 6" in text
        st, untouched, _ = raw([0, 2, 1], [0, 1], [1.0, 1.0], 2, [3, 2], 4)
        assert st == _capi.ERR_INVALID_ARGUMENT and untouched                                # a decreasing indptr
        st, untouched, _ = raw([0], [], [], 0, [1], 4)                                       # nq == 0: nothing enqueued, nothing written
        assert st == 0 and untouched
        st, untouched, _ = raw([0, 1, 2], [0, 1], [1.0, 1.0], 2, [3, 2], 4, ef=[0, 7])       # and a good call, ef given
        assert st == 0 and not untouched
        with pytest.raises(NeumannGpuError) as e:
            g.search_sparse_multi([0, 1], [6], [0.0], [3])                                   # checked before the zero is dropped
        assert e.value.status == _capi.ERR_INVALID_ARGUMENT
        with pytest.raises(NeumannGpuError):
            g.search_sparse_multi([0, 1], [1], [1.0], [3, 4])                                # one k per query
        ids, sc, cnt = g.search_sparse_multi([0], [], [], [], kstride=3)
        assert ids.shape == (0, 3) and cnt.size == 0


# ---- 5. long queries: 10, exactly 4096 and 5000 stored entries in one call ------------------------------------------------------------------
@pytest.mark.parametrize("metric", [ho.COSINE, ho.DOT_PRODUCT])
def test_long_queries_at_8192_dimensions(metric):
    rng = np.random.default_rng(8192)
    dim, n = 8192, 64
    rows = rng.standard_normal((n, dim)).astype(F)
    rows[rng.random(rows.shape) < 0.5] = 0.0
    o = ho.build(rows, o_cfg(metric))
    small = np.zeros(dim, dtype=F)
    small[rng.choice(dim, 10, replace=False)] = F(1.5)
    limit = np.zeros(dim, dtype=F)
    limit[rng.choice(dim, 4096, replace=False)] = F(-0.75)       # exactly what fits: walked on the device
    big = np.zeros(dim, dtype=F)
    big[rng.choice(dim, 5000, replace=False)] = rng.standard_normal(5000).astype(F)   # walked on the host, into the caller's row
    from neumann_amd import GpuHnsw
    with GpuHnsw(dim, g_cfg(metric)) as g:
        g.insert(rows)
        csr = g.sparse_from_dense(np.stack([small, limit, big]))
        assert np.diff(csr[0].astype(np.int64)).tolist() == [10, 4096, 5000]
        check_multi(g, o, "dense", dim, csr, np.array([10, 3, 7], np.uint32), np.array([50, 0, 200], np.uint32), 12, ("long", metric),
                    host_walked=(2,))
