"""The key layer, neumann_amd.CacheIndex (nmn_cache_index_*, include/neumann_cache.h), against tests/_cache_index_oracle.py: every
return of a scripted life of an index — node ids, answers (keys, order, similarity bits), len / contains / keys / memory_stats /
get_embedding — the reference's own CacheIndex tests restated (tensor_cache/src/index.rs:472 onward), the surprises of the key maps,
and eight threads at once."""
import math
import threading

import numpy as np
import pytest

from tests import _cache_index_oracle as co
from tests import _hnsw_mixed_oracle as mo
from tests import _hnsw_oracle as ho
from tests import _xmetric_oracle as xo
from tests.test_gpu_hnsw_cache_search import ACOS, NINE, SIM_TOL, g_config, g_metric

pytestmark = pytest.mark.gpu
F = np.float32


def create_test_vector(dim, seed):
    """index.rs:457-464"""
    return np.array([math.sin(float(F(F(seed * 31 + i * 17) * F(0.0001)))) for i in range(dim)], dtype=F)


class Pair:
    """the oracle and the library side by side: every call goes to both, and the returns must agree"""

    def __init__(self, dim, cfg=None, metric=None):
        from neumann_amd import CacheIndex
        self.o = co.CacheIndex(dim, cfg, metric)
        self.g = CacheIndex(dim, g_config(cfg) if cfg else None, g_metric(metric) if metric else None)

    def close(self):
        self.g.close()

    def insert(self, key, v):
        a, b = self.o.insert(key, v), self.g.insert(key, v)
        assert a == b, (key, a, b)
        return a

    def insert_sparse(self, key, sv):
        a, b = self.o.insert_sparse(key, sv), self.g.insert_sparse(key, sv.positions, sv.values)
        assert a == b, (key, a, b)
        return a

    def insert_auto(self, key, v, t):
        a, b = self.o.insert_auto(key, v, t), self.g.insert_auto(key, v, t)
        assert a == b and self.o.get_embedding(key)[0] == self.g.get_embedding(key)[0], (key, t)
        return a

    def _same(self, want, got, metric, what):
        assert [k for k, _ in got] == [k for k, _ in want], (what, got, want)
        for (_, a), (_, b) in zip(got, want):
            if metric.kind in ACOS:
                assert abs(float(a) - float(b)) <= SIM_TOL, what
            else:
                assert F(a).tobytes() == F(b).tobytes(), (what, a, b)
        return got

    def search(self, q, k, thr, metric=None):
        if metric is None:
            return self._same(self.o.search(q, k, thr), self.g.search(q, k, thr), self.o.distance_metric, ("search", k, thr))
        return self._same(self.o.search_with_metric(q, k, thr, metric), self.g.search_with_metric(q, k, thr, g_metric(metric)), metric,
                          ("search_with_metric", metric, k, thr))

    def search_sparse(self, sv, k, thr, metric=None):
        if metric is None:
            return self._same(self.o.search_sparse(sv, k, thr), self.g.search_sparse(sv.positions, sv.values, k, thr),
                              self.o.distance_metric, ("search_sparse", k, thr))
        return self._same(self.o.search_sparse_with_metric(sv, k, thr, metric),
                          self.g.search_sparse_with_metric(sv.positions, sv.values, k, thr, g_metric(metric)), metric,
                          ("search_sparse_with_metric", metric, k, thr))

    def remove(self, key):
        a, b = self.o.remove(key), self.g.remove(key)
        assert a == b
        return a

    def clear(self):
        self.o.clear()
        self.g.clear()

    def state(self):
        assert len(self.g) == len(self.o) and self.g.is_empty() == self.o.is_empty()
        assert sorted(self.g.keys()) == sorted(self.o.keys())
        for key in self.o.keys() + ["no-such-key"]:
            assert self.g.contains(key) == self.o.contains(key)
            a, b = self.o.get_embedding(key), self.g.get_embedding(key)
            assert (a is None) == (b is None)
            if a is None:
                continue
            assert a[0] == b[0], key
            if a[0] == "dense":
                assert np.array_equal(a[1], b[1])
            else:
                assert a[1].positions == b[1][0].tolist() and np.array_equal(np.asarray(a[1].values, dtype=F), b[1][1])
        ms, want = self.g.memory_stats(), self.o.memory_stats()
        assert {k: ms[k] for k in want} == want


@pytest.fixture
def pair3():
    p = Pair(3)
    yield p
    p.close()


# ---- the reference's own tests, restated -------------------------------------------------------------------------------------------
def test_insert_search_threshold_remove_and_empty(pair3):
    p = pair3
    assert p.search([1.0, 0.0, 0.0], 5, 0.0) == [] and p.g.is_empty()                       # test_empty_search, test_is_empty
    p.insert("key1", [1.0, 0.0, 0.0])
    p.insert("key2", [0.0, 1.0, 0.0])
    p.insert("key3", [0.9, 0.1, 0.0])
    res = p.search([1.0, 0.0, 0.0], 2, 0.5)                                                 # test_insert_and_search
    assert [k for k, _ in res] == ["key1", "key3"] and res[0][1] == F(1.0)
    assert [k for k, _ in p.search([1.0, 0.0, 0.0], 5, 0.999)] == ["key1"]                  # test_threshold_filtering
    assert p.g.contains("key1") and p.remove("key1") and not p.g.contains("key1") and len(p.g) == 2   # test_remove, test_contains
    assert "key1" not in [k for k, _ in p.search([1.0, 0.0, 0.0], 5, 0.0)]
    assert not p.remove("nonexistent")                                                      # test_remove_nonexistent
    assert p.g.dimension == 3                                                               # test_dimension
    p.state()


def test_dimension_mismatches(pair3):
    from neumann_amd import _capi
    g = pair3.g
    for call in (lambda: g.insert("k", [1.0, 0.0]), lambda: g.search([1.0, 0.0], 5, 0.0), lambda: g.insert_auto("k", [1.0, 0.0], 0.5),
                 lambda: g.insert_auto("k", [0.0, 0.0, 0.0, 1.0], 0.5), lambda: g.search([1.0, 0.0, 0.0, 0.0], 0, 0.0)):
        with pytest.raises(_capi.NeumannGpuError) as e:
            call()
        assert e.value.status == _capi.ERR_DIMENSION_MISMATCH and "expected 3, got" in str(e.value)
    with pytest.raises(_capi.NeumannGpuError) as e:
        g.insert_sparse("k", [3], [1.0])                                                    # a position the dimension does not hold
    assert "index 3 out of bounds for dimension 3" in str(e.value)
    with pytest.raises(_capi.NeumannGpuError):
        g.search_sparse([7], [1.0], 3, 0.0)
    assert len(g) == 0 and g.keys() == []


def test_many_vectors_keys_config_and_clear():
    cfg = ho.HNSWConfig.high_speed()                                                       # test_with_config
    p = Pair(128, cfg)
    try:
        for i in range(100):                                                                # test_many_vectors
            p.insert(f"key{i}", create_test_vector(128, i))
        res = p.search(create_test_vector(128, 50), 5, 0.9)
        assert len(res) == 5
        assert len(p.g) == 100 and sorted(p.g.keys()) == sorted(f"key{i}" for i in range(100))   # test_keys
        p.state()
        first = [p.o.index.levels[0], p.o.index.levels[1]]
        p.clear()                                                                           # test_clear
        assert len(p.g) == 0 and p.g.is_empty() and p.search(create_test_vector(128, 50), 5, 0.0) == []
        for i in range(100):    # identical ids and answers as a fresh index: ids from 0, the first levels drawn again
            assert p.insert(f"again{i}", create_test_vector(128, i)) == i
        assert [p.o.index.levels[0], p.o.index.levels[1]] == first
        assert [k for k, _ in p.search(create_test_vector(128, 50), 5, 0.9)] == [k.replace("key", "again") for k, _ in res]
        p.state()
    finally:
        p.close()


def test_sparse_auto_mixed_memory_stats_and_get_embedding():
    p = Pair(10)
    try:
        sv = mo.SparseVector.from_parts(10, [0, 5], [1.0, 0.5])                             # test_insert_sparse_and_search
        p.insert_sparse("sparse1", sv)
        assert [k for k, _ in p.search_sparse(sv, 5, 0.9)] == ["sparse1"]
        dense = np.array([1.0, 0.5, 0.3, 0.2, 0.1, 0.4, 0.6, 0.7, 0.8, 0.9], dtype=F)       # test_insert_auto_dense
        p.insert_auto("dense", dense, 0.7)
        sparse = np.zeros(10, dtype=F)                                                       # test_insert_auto_sparse
        sparse[[0, 9]] = [1.0, 0.5]
        p.insert_auto("auto-sparse", sparse, 0.7)
        assert p.g.get_embedding("dense")[0] == "dense" and p.g.get_embedding("auto-sparse")[0] == "sparse"
        for t in (0.0, 0.5, 1.0):                                                            # insert_auto at 0.0, 0.5 and 1.0
            half = np.zeros(10, dtype=F)
            half[:5] = 1.0
            p.insert_auto(f"half-{t}", half, t)
            p.insert_auto(f"zero-{t}", np.zeros(10, dtype=F), t)
        assert [p.g.get_embedding(f"half-{t}")[0] for t in (0.0, 0.5, 1.0)] == ["sparse", "sparse", "dense"]
        assert [p.g.get_embedding(f"zero-{t}")[0] for t in (0.0, 0.5, 1.0)] == ["sparse"] * 3
        ms = p.g.memory_stats()                                                              # test_memory_stats
        assert ms["total_nodes"] == 9 and ms["dense_count"] == 2 and ms["sparse_count"] == 7
        assert p.g.get_embedding("nonexistent") is None                                      # test_get_embedding
        for metric in NINE:                                                                  # test_mixed_dense_sparse_search, the overrides
            p.search(dense, 4, -1.0, metric)
            p.search_sparse(sv, 4, -1.0, metric)
            p.search_sparse(mo.SparseVector.from_parts(10, [5, 0, 5], [2.0, 1.0, -1.0]), 4, -1.0, metric)   # a duplicated position
        p.state()
    finally:
        p.close()


def test_configured_metric_and_ranking():
    p = Pair(4, None, xo.Metric(xo.JACCARD))                                                # test_with_metric_jaccard
    try:
        assert p.g.metric().name == "Jaccard"
        p.insert("a", [1.0, 2.0, 0.0, 0.0])
        p.insert("b", [0.0, 0.0, 3.0, 4.0])
        p.insert("c", [10.0, 0.0, 0.0, 0.0])
        res = p.search([1.0, 1.0, 0.0, 0.0], 3, 0.0)
        assert res[0] == ("a", F(1.0))
        cos = p.search([1.0, 1.0, 0.0, 0.0], 3, 0.0, xo.Metric(xo.COSINE))                  # test_search_with_metric_override
        assert [k for k, _ in cos][:2] == ["a", "c"]
        p.search([1.0, 1.0, 0.0, 0.0], 3, 0.0, xo.Metric(xo.EUCLIDEAN))                     # test_metric_affects_ranking
        p.state()
    finally:
        p.close()


# ---- the surprises of the key maps ---------------------------------------------------------------------------------------------------
def test_reinsert_and_remove_surprises(pair3):
    p = pair3
    assert p.insert("a", [1.0, 0.0, 0.0]) == 0
    assert p.insert("a", [0.9, 0.1, 0.0]) == 1                                              # test_reinsert_same_key
    assert len(p.g) == 1 and p.g.keys() == ["a"]
    assert [k for k, _ in p.search([1.0, 0.0, 0.0], 5, -1.0)] == ["a", "a"]                 # the old node keeps answering
    hnsw = p.g._lib.nmn_cache_index_hnsw(p.g._c)
    assert [p.g._lib.nmn_hnsw_node_live(hnsw, i) for i in range(3)] == [1, 1, -1]
    assert p.remove("a") and not p.g.contains("a") and len(p.g) == 0
    res = p.search([1.0, 0.0, 0.0], 5, -1.0)
    assert res == [("a", F(1.0))]                                                           # the orphan still answers
    assert [p.g._lib.nmn_hnsw_node_live(hnsw, i) for i in range(2)] == [1, 0]               # the mask is node_to_key
    p.insert("b", [0.0, 0.0, 1.0])
    assert p.search([1.0, 0.0, 0.0], 0, -1.0) == []                                         # k == 0
    assert len(p.search([1.0, 0.0, 0.0], 4_000_000_000, -1.0)) == 2                         # a k far beyond the index: every live node
    assert p.search([1.0, 0.0, 0.0], 5, math.nan) == []
    p.state()


# ---- eight threads ---------------------------------------------------------------------------------------------------------------------
def test_eight_threads_insert_remove_and_search():
    from neumann_amd import CacheIndex, ExtendedDistanceMetric as M
    dim, T, per = 16, 8, 30
    rng = np.random.default_rng(8)
    rows = rng.standard_normal((T, per, dim)).astype(F)
    rows[:, 1::3, ::2] = 0.0
    g = CacheIndex(dim)
    o = co.CacheIndex(dim)
    errs = []
    answers = [[] for _ in range(T)]
    start = threading.Barrier(T)

    def script(t):
        """thread t's own keys: insert all (every third by insert_auto), re-insert a few, remove every fourth"""
        for i in range(per):
            yield ("auto" if i % 3 == 1 else "insert"), f"t{t}-{i}", rows[t, i]
        for i in range(0, per, 5):
            yield "insert", f"t{t}-{i}", rows[t, (i + 1) % per]
        for i in range(0, per, 4):
            yield "remove", f"t{t}-{i}", None

    def work(t):
        try:
            start.wait()
            for n, (op, key, v) in enumerate(script(t)):
                if op == "insert":
                    g.insert(key, v)
                elif op == "auto":
                    g.insert_auto(key, v, 0.4)
                else:
                    assert g.remove(key)
                if n % 3 == 0:
                    answers[t].append((g.search_with_metric(rows[t, n % per], 4, 0.2, M(n % 9)),
                                       g.search_sparse(np.flatnonzero(rows[t, n % per]), rows[t, n % per][rows[t, n % per] != 0], 3, 0.2)))
        except Exception as e:  # noqa: BLE001
            errs.append(e)

    th = [threading.Thread(target=work, args=(t,)) for t in range(T)]
    for x in th:
        x.start()
    for x in th:
        x.join()
    try:
        assert not errs, errs
        ever = {f"t{t}-{i}" for t in range(T) for i in range(per)}
        for t in range(T):
            for dense, sparse in answers[t]:
                for res, k in ((dense, 4), (sparse, 3)):
                    sims = [float(s) for _, s in res]
                    assert len(res) <= k and all(key in ever for key, _ in res)
                    assert sims == sorted(sims, reverse=True) and all(s >= F(0.2) for s in sims)
        for t in range(T):   # the quiescent state: what the same calls leave in the oracle, thread after thread
            for op, key, v in script(t):
                if op == "insert":
                    o.insert(key, v)
                elif op == "auto":
                    o.insert_auto(key, v, 0.4)
                else:
                    o.remove(key)
        assert len(g) == len(o) and sorted(g.keys()) == sorted(o.keys())
        for key in ever:
            assert g.contains(key) == o.contains(key)
            a, b = o.get_embedding(key), g.get_embedding(key)
            assert (a is None) == (b is None) and (a is None or a[0] == b[0])
            if a is not None and a[0] == "dense":
                assert np.array_equal(a[1], b[1])
        ms, want = g.memory_stats(), o.memory_stats()
        assert {k: ms[k] for k in want} == want
        hnsw = g._lib.nmn_cache_index_hnsw(g._c)                      # the mask equals "a key answers for the node"
        live = sum(g._lib.nmn_hnsw_node_live(hnsw, i) for i in range(ms["total_nodes"]))
        assert live == len(o.node_to_key)
    finally:
        g.close()
