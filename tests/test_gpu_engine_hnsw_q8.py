"""VectorEngine.build_hnsw_index_with_options (vector_engine/src/lib.rs:2423-2470) with HNSWBuildOptions::memory_optimized —
quantized storage — through the engine mirror: the graph and search_with_hnsw against tests/_hnsw_q8_oracle.py, and
search_with_hnsw_and_metric against the composition of that oracle's walk and tests/_xmetric_oracle.py over the engine's CURRENT
f32 vectors."""
import functools

import numpy as np
import pytest

from tests import _hnsw_oracle as ho
from tests import _hnsw_q8_oracle as q8
from tests import _xmetric_oracle as xo

pytestmark = pytest.mark.gpu
F = np.float32
N, DIM = 300, 24


@pytest.fixture
def E():
    from neumann_amd import engine
    return engine


@functools.lru_cache(maxsize=None)
def corpus():
    rng = np.random.default_rng(0x51)
    rows = (rng.standard_normal((N, DIM)) + 2.0 * rng.standard_normal((5, DIM))[rng.integers(0, 5, N)]).astype(F)
    for i in range(6, N, 6):
        rows[i] = rows[rng.integers(0, i)]      # duplicates: equal scores, the stable order decides
    queries = rng.standard_normal((8, DIM)).astype(F)
    queries[:3] = rows[[10, 100, 200]]
    return rows, queries


def filled(E):
    rows, _ = corpus()
    eng = E.VectorEngine()
    for i in np.random.default_rng(2).permutation(N):   # stored in scrambled order
        eng.store_embedding(f"key{i:05d}", rows[i])
    return eng


@functools.lru_cache(maxsize=None)
def oracle(order):
    return q8.build(corpus()[0][list(order)], ho.HNSWConfig.high_speed())   # memory_optimized = Quantized + high_speed


def g_metric(m):
    from neumann_amd import ExtendedDistanceMetric, GeometricConfig
    if m.kind == xo.COMPOSITE:
        return ExtendedDistanceMetric.Composite(GeometricConfig(*[float(w) for w in m.config.weights()]))
    return ExtendedDistanceMetric(m.kind)


def as_bits(res):
    return [(r.key, F(r.score).tobytes()) for r in res]


def want_bits(res):
    return [(k, F(s).tobytes()) for k, s in res]


def test_memory_optimized_builds_the_quantized_oracles_graph(E):
    from neumann_amd import HNSWBuildOptions
    eng = filled(E)
    rows, queries = corpus()
    index, key_mapping = eng.build_hnsw_index_with_options(HNSWBuildOptions.memory_optimized())
    assert key_mapping == eng.list_keys() and len(index) == N
    o = oracle(tuple(int(k[3:]) for k in key_mapping))
    g = index.gpu()
    assert g.storage == "quantized" and g.vectors() is None
    assert g.memory_stats()["quantized_count"] == N and g.memory_stats()["embedding_bytes"] == N * (16 + DIM)
    assert g.entry_point == o.entry_point and g.max_layer == o.max_layer and g.levels().tolist() == o.levels
    for node in range(N):
        for layer in range(o.levels[node] + 1):
            assert g.neighbors(node, layer).tolist() == o.neighbors[node][layer], (node, layer)
        codes, scale, mn = g.quantized_row(node)
        assert np.array_equal(codes, o.codes[node]) and scale.tobytes() == o.scale[node].tobytes() and mn.tobytes() == o.min_val[node].tobytes()
    for q in queries:
        for top_k in (1, 7, N + 5):
            got = eng.search_with_hnsw(index, key_mapping, q, top_k)
            assert as_bits(got) == want_bits(ho.search_with_hnsw(o, key_mapping, q, top_k)), top_k


def test_default_options_are_build_hnsw_index(E):
    from neumann_amd import HNSWBuildOptions
    eng = filled(E)
    a, keys_a = eng.build_hnsw_index_with_options()
    b, keys_b = eng.build_hnsw_index_with_options(HNSWBuildOptions.default().with_storage("dense"))
    c, keys_c = eng.build_hnsw_index_default()
    assert keys_a == keys_b == keys_c
    ga, gb, gc = a.gpu(), b.gpu(), c.gpu()
    assert ga.storage == gb.storage == gc.storage == "dense"
    assert ga.levels().tolist() == gc.levels().tolist()
    for node in range(0, N, 7):
        assert ga.neighbors(node, 0).tolist() == gb.neighbors(node, 0).tolist() == gc.neighbors(node, 0).tolist()
    q = corpus()[1][4]
    assert as_bits(eng.search_with_hnsw(a, keys_a, q, 9)) == as_bits(eng.search_with_hnsw(c, keys_c, q, 9))


@pytest.mark.parametrize("metric", [xo.Metric(xo.COSINE), xo.Metric(xo.COMPOSITE, xo.GeometricConfig.default())], ids=["cosine", "composite"])
def test_search_with_hnsw_and_metric_reranks_with_the_current_vectors(E, metric):
    """the quantized oracle's walk for c = max(2 top_k, 10) candidates, then the re-rank over the engine's current f32 vectors —
    before and after overwriting one vector and deleting another"""
    from neumann_amd import HNSWBuildOptions
    eng = filled(E)
    rows, queries = corpus()
    index, key_mapping = eng.build_hnsw_index_with_options(HNSWBuildOptions.memory_optimized())
    o = oracle(tuple(int(k[3:]) for k in key_mapping))
    vecs = {f"key{i:05d}": rows[i] for i in range(N)}
    for q in queries:
        for top_k in (1, 8):
            got = eng.search_with_hnsw_and_metric(index, key_mapping, q, top_k, g_metric(metric))
            assert as_bits(got) == want_bits(xo.search_with_hnsw_and_metric(o, key_mapping, vecs, q, top_k, metric)), top_k
    q = queries[1]
    before = eng.search_with_hnsw_and_metric(index, key_mapping, q, 8, g_metric(metric))
    victim, moved = before[1].key, before[3].key
    new = (q + F(0.001)).astype(F)
    eng.store_embedding(moved, new)
    vecs[moved] = new
    eng.delete_embedding(victim)
    del vecs[victim]
    after = eng.search_with_hnsw_and_metric(index, key_mapping, q, 8, g_metric(metric))
    assert victim not in [r.key for r in after]
    assert as_bits(after) == want_bits(xo.search_with_hnsw_and_metric(o, key_mapping, vecs, q, 8, metric))
    short = key_mapping[:150]                                                  # a caller-supplied mapping
    got = eng.search_with_hnsw_and_metric(index, short, q, 8, g_metric(metric))
    assert as_bits(got) == want_bits(xo.search_with_hnsw_and_metric(o, short, vecs, q, 8, metric))


def test_dimension_and_empty_engine_rules(E):
    from neumann_amd import HNSWBuildOptions
    opt = HNSWBuildOptions.memory_optimized
    eng = E.VectorEngine()
    index, key_mapping = eng.build_hnsw_index_with_options(opt())             # an empty engine gives an empty index
    assert len(index) == 0 and key_mapping == [] and index.gpu() is None
    assert eng.search_with_hnsw(index, key_mapping, [1.0], 3) == []
    eng.store_embedding("a", np.ones(8, F))
    eng.store_embedding("b", np.ones(6, F))
    first = len(eng.get_embedding(eng.list_keys()[0]))
    with pytest.raises(E.VectorError) as e:                                   # lib.rs:2458-2463
        eng.build_hnsw_index_with_options(opt())
    assert e.value.kind == "DimensionMismatch" and str(e.value) == f"Dimension mismatch: expected {first}, got {14 - first}"
    eng = E.VectorEngine(E.VectorEngineConfig(max_dimension=4))
    eng.store_embedding("a", np.ones(4, F))
    index, _ = eng.build_hnsw_index_with_options(opt())
    assert len(index) == 1
    with pytest.raises(E.VectorError) as e:
        eng.search_with_hnsw(index, index.keys, np.ones(5, F), 1)
    assert e.value.kind == "DimensionMismatch"


def test_sparse_optimized_is_refused(E):
    from neumann_amd import HNSWBuildOptions
    eng = filled(E)
    with pytest.raises(E.VectorError) as e:
        eng.build_hnsw_index_with_options(HNSWBuildOptions.sparse_optimized())
    assert e.value.kind == "ConfigurationError"
    with pytest.raises(E.VectorError) as e:
        eng.build_hnsw_index_with_options(HNSWBuildOptions.new().with_storage("auto").with_sparsity_threshold(0.7))
    assert e.value.kind == "ConfigurationError"
