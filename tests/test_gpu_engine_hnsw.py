"""VectorEngine.build_hnsw_index / search_with_hnsw / estimate_hnsw_memory (vector_engine/src/lib.rs:2378-2550) through the
engine mirror, against tests/_hnsw_oracle.py and the reference's own tests of them."""
import numpy as np
import pytest

from tests import _hnsw_oracle as ho

pytestmark = pytest.mark.gpu
F = np.float32


@pytest.fixture
def E():
    from neumann_amd import engine
    return engine


def create_test_vector(dim, seed):  # tests::create_test_vector (lib.rs:4029-4038)
    i = np.arange(dim, dtype=np.int64)
    x = (seed * 31 + i * 17).astype(F)
    return (np.sin(x * F(0.0001), dtype=F) * ((seed + i).astype(F) * F(0.001))).astype(F)


def filled(E, n, dim, seed=5, config=None):
    rng = np.random.default_rng(seed)
    rows = (rng.standard_normal((n, dim)) + 2.0 * rng.standard_normal((5, dim))[rng.integers(0, 5, n)]).astype(F)
    eng = E.VectorEngine(config)
    for i in rng.permutation(n):  # stored in scrambled order
        eng.store_embedding(f"key{i:05d}", rows[i])
    return eng, rows


def assert_graph(g, o):
    assert len(g) == len(o) and g.entry_point == o.entry_point and g.max_layer == o.max_layer
    assert g.levels().tolist() == o.levels
    for node in range(len(o)):
        for layer in range(o.levels[node] + 1):
            assert g.neighbors(node, layer).tolist() == o.neighbors[node][layer], (node, layer)


def test_engine_search_with_hnsw(E):  # lib.rs:4643-4667
    eng = E.VectorEngine()
    for i in range(100):
        eng.store_embedding(f"vec{i}", create_test_vector(32, i))
    index, key_mapping = eng.build_hnsw_index_default()
    res = eng.search_with_hnsw(index, key_mapping, create_test_vector(32, 42), 5)
    assert len(res) == 5
    assert any("42" in r.key for r in res)
    # ... and bit for bit what the reference's algorithm returns for the same key order
    rows = np.stack([create_test_vector(32, int(k[3:])) for k in key_mapping])
    o = ho.build(rows)
    want = ho.search_with_hnsw(o, key_mapping, create_test_vector(32, 42), 5)
    assert [(r.key, np.float32(r.score).tobytes()) for r in res] == [(k, np.float32(s).tobytes()) for k, s in want]


def test_engine_hnsw_error_cases(E):  # lib.rs:4670-4687
    eng = E.VectorEngine()
    index, key_mapping = eng.build_hnsw_index_default()  # an empty engine gives an empty index
    assert len(index) == 0 and key_mapping == [] and index.gpu() is None
    with pytest.raises(E.VectorError) as e:
        eng.search_with_hnsw(index, key_mapping, [], 5)
    assert e.value.kind == "EmptyVector" and str(e.value) == "Empty vector provided"
    with pytest.raises(E.VectorError) as e:
        eng.search_with_hnsw(index, key_mapping, [1.0], 0)
    assert e.value.kind == "InvalidTopK" and str(e.value) == "Invalid top_k value (must be > 0)"
    assert eng.search_with_hnsw(index, key_mapping, [1.0], 3) == []


@pytest.mark.parametrize("metric", [ho.COSINE, ho.EUCLIDEAN, ho.DOT_PRODUCT])
def test_build_uses_list_keys_order_and_the_reference_graph(E, metric):
    from neumann_amd import HNSWConfig
    eng, rows = filled(E, 300, 24)
    index, key_mapping = eng.build_hnsw_index(HNSWConfig.high_speed().with_distance_metric(metric))
    assert key_mapping == eng.list_keys() and len(index) == 300
    order = [int(k[3:]) for k in key_mapping]
    o = ho.build(rows[order], ho.HNSWConfig.high_speed().with_distance_metric(metric))
    assert_graph(index.gpu(), o)
    rng = np.random.default_rng(9)
    for q in rng.standard_normal((20, 24)).astype(F):
        got = eng.search_with_hnsw(index, key_mapping, q, 7)
        want = ho.search_with_hnsw(o, key_mapping, q, 7)
        assert [(r.key, np.float32(r.score).tobytes()) for r in got] == [(k, np.float32(s).tobytes()) for k, s in want]
    # node ids past a shorter caller-supplied mapping are dropped (lib.rs:2543-2548)
    short = key_mapping[:150]
    got = eng.search_with_hnsw(index, short, rows[0], 10)
    want = ho.search_with_hnsw(o, short, rows[0], 10)
    assert [r.key for r in got] == [k for k, _ in want]
    # a snapshot: later stores do not change it
    eng.store_embedding("later", rows[0])
    assert len(index) == 300 and [r.key for r in eng.search_with_hnsw(index, key_mapping, rows[0], 10)] == \
        [k for k, _ in ho.search_with_hnsw(o, key_mapping, rows[0], 10)]


def test_dimension_errors_carry_the_reference_texts(E):
    eng = E.VectorEngine()
    eng.store_embedding("a", np.ones(8, F))
    eng.store_embedding("b", np.ones(6, F))
    first = len(eng.get_embedding(eng.list_keys()[0]))
    other = 14 - first
    with pytest.raises(E.VectorError) as e:  # lib.rs:2458-2463
        eng.build_hnsw_index_default()
    assert e.value.kind == "DimensionMismatch" and str(e.value) == f"Dimension mismatch: expected {first}, got {other}"
    eng = E.VectorEngine(E.VectorEngineConfig(max_dimension=16))
    eng.store_embedding("a", np.ones(16, F))
    index, _ = eng.build_hnsw_index_default()
    assert len(index) == 1
    with pytest.raises(E.VectorError) as e:
        eng.search_with_hnsw(index, index.keys, np.ones(5, F), 1)
    assert e.value.kind == "DimensionMismatch"


def test_out_of_scope_strategies_are_refused(E):
    from neumann_amd import HNSWConfig
    eng, _ = filled(E, 10, 8)
    for storage in ("auto", "quantized"):
        with pytest.raises(E.VectorError) as e:
            eng.build_hnsw_index(HNSWConfig(storage=storage))
        assert e.value.kind == "ConfigurationError"


def test_estimate_hnsw_memory(E):  # lib.rs:2489-2509
    eng = E.VectorEngine()
    assert eng.estimate_hnsw_memory() == 0
    eng, _ = filled(E, 123, 40)
    assert eng.estimate_hnsw_memory() == 123 * 40 * 4 + 123 * 16 * 2 * 8 + 123 * 32 == ho.estimate_hnsw_memory(123, 40)


def test_recall_against_search_similar_is_the_oracles(E):
    """recall@10 of search_with_hnsw against search_similar on the same engine.  The graph is the reference's, so the recall asserted
    is the one the ORACLE reaches on this corpus (against the exhaustive ranking), not a chosen constant."""
    eng, rows = filled(E, 1200, 32, seed=21)
    index, key_mapping = eng.build_hnsw_index_default()
    order = [int(k[3:]) for k in key_mapping]
    o = ho.build(rows[order])
    rng = np.random.default_rng(4)
    Q = (rows[rng.integers(0, 1200, 50)] + 0.3 * rng.standard_normal((50, 32))).astype(F)
    hit = hit_o = 0
    for q in Q:
        exact = {r.key for r in eng.search_similar(q, 10)}
        hit += len(exact & {r.key for r in eng.search_with_hnsw(index, key_mapping, q, 10)})
        hit_o += len(exact & {k for k, _ in ho.search_with_hnsw(o, key_mapping, q, 10)})
    print(f"recall@10 of search_with_hnsw against search_similar, 1200 x 32, default config: {hit / 500:.3f} (oracle: {hit_o / 500:.3f})")
    assert hit == hit_o
