"""VectorEngine.search_with_hnsw_and_metric (vector_engine/src/lib.rs:2560-2619) through the engine mirror, against
tests/_xmetric_oracle.py and the reference's own tests of it (lib.rs:5455-5536, 5853-5944)."""
import functools

import numpy as np
import pytest

from tests import _hnsw_oracle as ho
from tests import _xmetric_oracle as xo

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


def g_metric(m):
    from neumann_amd import ExtendedDistanceMetric, GeometricConfig
    if m.kind == xo.COMPOSITE:
        return ExtendedDistanceMetric.Composite(GeometricConfig(*[float(w) for w in m.config.weights()]))
    return ExtendedDistanceMetric(m.kind)


def as_bits(res):
    return [(r.key, F(r.score).tobytes()) for r in res]


def want_bits(res):
    return [(k, F(s).tobytes()) for k, s in res]


def small_engine(E, named):
    eng = E.VectorEngine()
    for k, v in named:
        eng.store_embedding(k, np.asarray(v, dtype=F))
    index, key_mapping = eng.build_hnsw_index_default()
    return eng, index, key_mapping


def oracle_for(eng, key_mapping):
    vecs = {k: np.asarray(eng.get_embedding(k), dtype=F) for k in key_mapping}
    return ho.build(np.stack([vecs[k] for k in key_mapping])), vecs


# ---- the reference's own tests ------------------------------------------------------------------------------------------------
def test_basic_cosine(E):  # lib.rs:5455-5480
    from neumann_amd import ExtendedDistanceMetric as M
    eng, index, key_mapping = small_engine(E, [(f"v{i}", create_test_vector(32, i)) for i in range(50)])
    q = create_test_vector(32, 25)
    res = eng.search_with_hnsw_and_metric(index, key_mapping, q, 5, M.Cosine)
    assert len(res) == 5 and any(r.key == "v25" for r in res)
    o, vecs = oracle_for(eng, key_mapping)
    assert as_bits(res) == want_bits(xo.search_with_hnsw_and_metric(o, key_mapping, vecs, q, 5, xo.Metric(xo.COSINE)))


@pytest.mark.parametrize("named,query,top_k,kind,first", [
    ([("a", [1.0, 0.0]), ("b", [2.0, 0.0]), ("c", [10.0, 0.0])], [1.0, 0.0], 3, xo.EUCLIDEAN, "a"),             # 5483-5504
    ([("a", [1.0, 0.0]), ("b", [0.707, 0.707]), ("c", [0.0, 1.0])], [1.0, 0.0], 3, xo.ANGULAR, "a"),            # 5853-5874
    ([("a", [1.0, 1.0, 0.0]), ("b", [1.0, 0.0, 0.0]), ("c", [0.0, 0.0, 1.0])], [1.0, 1.0, 0.0], 3, xo.JACCARD, "a"),  # 5877-5898
    ([("a", [1.0, 1.0, 0.0]), ("b", [1.0, 0.0, 0.0])], [1.0, 1.0, 0.0], 2, xo.OVERLAP, None),                    # 5901-5920
    ([("origin", [0.0, 0.0]), ("one", [1.0, 0.0]), ("two", [2.0, 0.0])], [0.0, 0.0], 3, xo.MANHATTAN, "origin"),  # 5923-5944
], ids=["euclidean", "angular", "jaccard", "overlap", "manhattan"])
def test_reference_engine_cases(E, named, query, top_k, kind, first):
    eng, index, key_mapping = small_engine(E, named)
    metric = xo.Metric(kind)
    res = eng.search_with_hnsw_and_metric(index, key_mapping, query, top_k, g_metric(metric))
    assert len(res) == top_k
    if first:
        assert res[0].key == first
    o, vecs = oracle_for(eng, key_mapping)
    want = xo.search_with_hnsw_and_metric(o, key_mapping, vecs, np.asarray(query, dtype=F), top_k, metric)
    assert [r.key for r in res] == [k for k, _ in want]
    if kind == xo.ANGULAR:
        assert max(abs(float(r.score) - float(s)) for r, (_, s) in zip(res, want)) <= 2.0 ** -22
    else:
        assert as_bits(res) == want_bits(want)


def test_error_cases(E):  # lib.rs:5507-5536
    from neumann_amd import ExtendedDistanceMetric as M
    eng = E.VectorEngine()
    index, key_mapping = eng.build_hnsw_index_default()
    with pytest.raises(E.VectorError) as e:
        eng.search_with_hnsw_and_metric(index, key_mapping, [], 5, M.Cosine)
    assert e.value.kind == "EmptyVector" and str(e.value) == "Empty vector provided"
    with pytest.raises(E.VectorError) as e:
        eng.search_with_hnsw_and_metric(index, key_mapping, [1.0], 0, M.Cosine)
    assert e.value.kind == "InvalidTopK" and str(e.value) == "Invalid top_k value (must be > 0)"
    assert eng.search_with_hnsw_and_metric(index, key_mapping, [1.0], 3, M.Cosine) == []
    with pytest.raises(E.VectorError) as e:
        eng.search_with_hnsw_and_metric(index, key_mapping, [1.0], 3, M(9))
    assert e.value.kind == "ConfigurationError"
    # no zero-magnitude rule here, unlike search_similar: a zero query is scored
    eng, index, key_mapping = small_engine(E, [("origin", [0.0, 0.0]), ("one", [1.0, 0.0])])
    res = eng.search_with_hnsw_and_metric(index, key_mapping, [0.0, 0.0], 2, M.Cosine)
    assert [F(r.score) for r in res] == [F(0.5), F(0.5)]


# ---- the two paths -------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def corpus300():
    rng = np.random.default_rng(77)
    rows = (rng.standard_normal((300, 16)) + 2.0 * rng.standard_normal((5, 16))[rng.integers(0, 5, 300)]).astype(F)
    rows[rng.random(rows.shape) < 0.3] = 0.0
    for i in range(6, 300, 6):
        rows[i] = rows[rng.integers(0, i)]  # duplicates: equal scores, the stable order decides
    queries = rng.standard_normal((6, 16)).astype(F)
    queries[:2] = rows[[10, 200]]
    return rows, queries


def engine300(E, config=None):
    rows, queries = corpus300()
    eng = E.VectorEngine(config)
    for i in np.random.default_rng(1).permutation(300):
        eng.store_embedding(f"key{i:05d}", rows[i])
    index, key_mapping = eng.build_hnsw_index_default()
    return eng, index, key_mapping, rows, queries


@functools.lru_cache(maxsize=None)
def oracle300(order):
    return ho.build(corpus300()[0][list(order)])


SEVEN = [xo.Metric(k) for k in (xo.COSINE, xo.JACCARD, xo.OVERLAP, xo.WEIGHTED_JACCARD, xo.EUCLIDEAN, xo.MANHATTAN)] + [
    xo.Metric(xo.COMPOSITE, xo.GeometricConfig.default())]


def test_fast_path_equals_changed_path_and_the_oracle(E):
    eng, index, key_mapping, rows, queries = engine300(E)
    o = oracle300(tuple(int(k[3:]) for k in key_mapping))
    vecs = {f"key{i:05d}": rows[i] for i in range(300)}
    fast = {}
    for metric in SEVEN + [xo.Metric(xo.ANGULAR)]:
        for qi, q in enumerate(queries):
            for top_k in (1, 7, 200):
                fast[(repr(metric), qi, top_k)] = eng.search_with_hnsw_and_metric(index, key_mapping, q, top_k, g_metric(metric))
    for metric in SEVEN:
        for qi, q in enumerate(queries[:3]):
            want = xo.search_with_hnsw_and_metric(o, key_mapping, vecs, q, 7, metric)
            assert as_bits(fast[(repr(metric), qi, 7)]) == want_bits(want), (metric, qi)
    # overwrite one stored vector with its own value: the write counter moves, nothing else does
    eng.store_embedding("key00010", rows[10])
    for metric in SEVEN + [xo.Metric(xo.ANGULAR)]:
        for qi, q in enumerate(queries):
            for top_k in (1, 7, 200):
                changed = eng.search_with_hnsw_and_metric(index, key_mapping, q, top_k, g_metric(metric))
                assert as_bits(changed) == as_bits(fast[(repr(metric), qi, top_k)]), (metric, qi, top_k)


def test_deleted_and_overwritten_candidates(E):
    eng, index, key_mapping, rows, queries = engine300(E)
    o = oracle300(tuple(int(k[3:]) for k in key_mapping))
    vecs = {f"key{i:05d}": rows[i] for i in range(300)}
    metric = xo.Metric(xo.EUCLIDEAN)
    q = queries[2]
    before = eng.search_with_hnsw_and_metric(index, key_mapping, q, 8, g_metric(metric))
    victim, moved = before[1].key, before[3].key
    # delete a key that was among the candidates: it is gone, the list is otherwise the oracle's
    eng.delete_embedding(victim)
    del vecs[victim]
    after = eng.search_with_hnsw_and_metric(index, key_mapping, q, 8, g_metric(metric))
    assert victim not in [r.key for r in after]
    assert as_bits(after) == want_bits(xo.search_with_hnsw_and_metric(o, key_mapping, vecs, q, 8, metric))
    # overwrite a candidate's vector with a different one: its score is the new vector's
    new = (q + F(0.001)).astype(F)
    eng.store_embedding(moved, new)
    vecs[moved] = new
    after = eng.search_with_hnsw_and_metric(index, key_mapping, q, 8, g_metric(metric))
    assert after[0].key == moved and F(after[0].score) == xo.score_dense(metric, q, new)[1]
    assert as_bits(after) == want_bits(xo.search_with_hnsw_and_metric(o, key_mapping, vecs, q, 8, metric))
    # ... of another length: zero-padded to the longer of the two
    short, long_ = np.asarray([1.0, -2.0, 0.5], dtype=F), np.concatenate([q, np.asarray([3.0, 0.0, 1.0], dtype=F)])
    for new in (short, long_):
        eng.store_embedding(moved, new)
        vecs[moved] = new
        for m in (metric, xo.Metric(xo.JACCARD), xo.Metric(xo.COMPOSITE, xo.GeometricConfig.default())):
            after = eng.search_with_hnsw_and_metric(index, key_mapping, q, 20, g_metric(m))
            assert as_bits(after) == want_bits(xo.search_with_hnsw_and_metric(o, key_mapping, vecs, q, 20, m)), (m, len(new))
    # clear: every key is gone
    eng.clear()
    assert eng.search_with_hnsw_and_metric(index, key_mapping, q, 8, g_metric(metric)) == []


def test_shorter_key_mapping_drops_ids_past_it(E):
    eng, index, key_mapping, rows, queries = engine300(E)
    o = oracle300(tuple(int(k[3:]) for k in key_mapping))
    vecs = {f"key{i:05d}": rows[i] for i in range(300)}
    metric = xo.Metric(xo.MANHATTAN)
    short = key_mapping[:120]
    for q in queries[:3]:
        res = eng.search_with_hnsw_and_metric(index, short, q, 10, g_metric(metric))
        want = xo.search_with_hnsw_and_metric(o, short, vecs, q, 10, metric)
        assert as_bits(res) == want_bits(want)
        assert all(r.key in short for r in res)
    full = [r.key for r in eng.search_with_hnsw_and_metric(index, key_mapping, queries[0], 10, g_metric(metric))]
    cut = [r.key for r in eng.search_with_hnsw_and_metric(index, short, queries[0], 10, g_metric(metric))]
    assert cut != full or all(k in short for k in full)


def test_dimension_mismatch_and_timeout(E):
    from neumann_amd import ExtendedDistanceMetric as M
    eng, index, key_mapping, rows, queries = engine300(E)
    with pytest.raises(E.VectorError) as e:
        eng.search_with_hnsw_and_metric(index, key_mapping, np.ones(5, F), 3, M.Cosine)
    assert e.value.kind == "DimensionMismatch" and str(e.value) == "Dimension mismatch: expected 16, got 5"
    with pytest.raises(E.VectorError) as e2:
        eng.search_with_hnsw(index, key_mapping, np.ones(5, F), 3)
    assert str(e2.value) == str(e.value)
    # the timeout error carries the operation name (lib.rs:2581-2586), on both paths
    eng, index, key_mapping, rows, queries = engine300(E, E.VectorEngineConfig(search_timeout=0.0))
    for _ in range(2):
        with pytest.raises(E.VectorError) as e:
            eng.search_with_hnsw_and_metric(index, key_mapping, queries[0], 3, M.Cosine)
        assert e.value.kind == "SearchTimeout" and "search_with_hnsw_and_metric" in str(e.value)
        eng.store_embedding("key00000", rows[0])
