"""The hnsw_cache hook of VectorEngine::search_similar / search_in_collection (vector_engine/src/lib.rs:1305-1334, 1622-1646,
1976-2001) through the engine mirror: the reference's fourteen cache tests restated one for one (lib.rs:9686-9944), parity with
tests/_hnsw_cache_oracle.py on the golden corpus (keys and score BITS), the invalidation table line by line, the fall-through
rules, ownership of the cached index, and concurrent callers."""
import os
import threading

import numpy as np
import pytest

from oracle import oracle_c as oc
from tests import _hnsw_cache_oracle as co
from tests import _hnsw_oracle as ho

pytestmark = pytest.mark.gpu
F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "hnsw_small.npz")
D = "_default"


@pytest.fixture
def E():
    from neumann_amd import engine
    return engine


def pairs(res):
    return [(r.key, F(r.score).tobytes()) for r in res]


def want_pairs(res):
    return [(k, F(s).tobytes()) for k, s in res]


def abc(E, rows=((1, 0, 0), (0, 1, 0), (0, 0, 1))):
    eng = E.VectorEngine()
    for key, v in zip("abcdefgh", rows):
        eng.store_embedding(key, list(map(float, v)))
    return eng


def empty_index(E):
    """`HNSWIndex::new()`: the index of an engine that holds nothing"""
    return E.VectorEngine().build_hnsw_index_default()[0]


# ---- the reference's fourteen (lib.rs:9686-9944) -------------------------------------------------------------------------------
def test_cache_hnsw_index_accelerates_search_similar(E):  # lib.rs:9688-9702
    eng = abc(E)
    eng.build_and_cache_index()
    res = eng.search_similar([1.0, 0.0, 0.0], 2)
    assert len(res) == 2 and res[0].key == "a"


def test_cache_hnsw_index_returns_correct_top_k(E):  # lib.rs:9705-9718
    eng = abc(E, ((1, 0, 0), (0.9, 0.1, 0), (0, 1, 0), (0, 0, 1)))
    eng.build_and_cache_index()
    res = eng.search_similar([1.0, 0.0, 0.0], 1)
    assert len(res) == 1 and res[0].key == "a"


def test_cache_invalidated_on_store_embedding(E):  # lib.rs:9721-9735
    eng = abc(E, ((1, 0, 0), (0, 1, 0)))
    eng.build_and_cache_index()
    assert eng.hnsw_cache_contains(D)
    eng.store_embedding("c", [0.0, 0.0, 1.0])
    assert not eng.hnsw_cache_contains(D)


def test_cache_invalidated_on_delete_embedding(E):  # lib.rs:9738-9749
    eng = abc(E, ((1, 0, 0), (0, 1, 0)))
    eng.build_and_cache_index()
    assert eng.hnsw_cache_contains(D)
    eng.delete_embedding("a")
    assert not eng.hnsw_cache_contains(D)


def test_cache_invalidated_on_store_in_collection(E):  # lib.rs:9752-9772
    eng = E.VectorEngine()
    eng.create_collection("test_coll")
    eng.store_in_collection("test_coll", "a", [1.0, 0.0, 0.0])
    eng.cache_hnsw_index("test_coll", empty_index(E), ["a"])
    assert eng.hnsw_cache_contains("test_coll")
    eng.store_in_collection("test_coll", "b", [0.0, 1.0, 0.0])
    assert not eng.hnsw_cache_contains("test_coll")


def test_cache_invalidated_on_delete_from_collection(E):  # lib.rs:9775-9791
    eng = E.VectorEngine()
    eng.create_collection("test_coll")
    eng.store_in_collection("test_coll", "a", [1.0, 0.0, 0.0])
    eng.cache_hnsw_index("test_coll", empty_index(E), ["a"])
    assert eng.hnsw_cache_contains("test_coll")
    eng.delete_from_collection("test_coll", "a")
    assert not eng.hnsw_cache_contains("test_coll")


def test_invalidate_hnsw_cache_nonexistent_collection(E):  # lib.rs:9794-9799
    E.VectorEngine().invalidate_hnsw_cache("nonexistent")


def test_cache_search_similar_empty_cache_falls_through(E):  # lib.rs:9802-9812
    eng = abc(E, ((1, 0, 0), (0, 1, 0)))
    res = eng.search_similar([1.0, 0.0, 0.0], 2)
    assert len(res) == 2 and res[0].key == "a"


def test_cache_search_in_collection_uses_cached_index(E):  # lib.rs:9815-9853
    eng = E.VectorEngine()
    eng.create_collection("docs")
    rows = {"d1": [1.0, 0.0, 0.0], "d2": [0.0, 1.0, 0.0], "d3": [0.0, 0.0, 1.0]}
    for k, v in rows.items():
        eng.store_in_collection("docs", k, v)
    # "build an HNSW index for the collection manually": the same rows through a scratch engine, mapped to the storage keys
    scratch = E.VectorEngine()
    for k, v in rows.items():
        scratch.store_embedding(k, v)
    index, keys = scratch.build_hnsw_index_default()
    eng.cache_hnsw_index("docs", index, [co.collection_embedding_prefix("docs") + k for k in keys])
    res = eng.search_in_collection("docs", [1.0, 0.0, 0.0], 2)
    assert len(res) == 2 and res[0].key == "d1"


def test_build_and_cache_index_empty_store(E):  # lib.rs:9856-9868
    eng = E.VectorEngine()
    eng.build_and_cache_index()
    assert eng.hnsw_cache_contains(D) and eng.hnsw_cache_keys(D) == []


def test_build_and_cache_index_search_results_match_brute_force(E):  # lib.rs:9871-9892
    eng = abc(E, ((1, 0, 0), (0.9, 0.1, 0), (0, 1, 0), (0, 0, 1)))
    brute = eng.search_similar([1.0, 0.0, 0.0], 4)
    eng.build_and_cache_index()
    cached = eng.search_similar([1.0, 0.0, 0.0], 4)
    assert len(brute) == len(cached) and brute[0].key == "a" and cached[0].key == "a"


def test_cache_manual_insert_and_invalidate(E):  # lib.rs:9895-9906
    eng = E.VectorEngine()
    eng.cache_hnsw_index("my_coll", empty_index(E), ["key1", "key2"])
    assert eng.hnsw_cache_contains("my_coll") and eng.hnsw_cache_keys("my_coll") == ["key1", "key2"]
    eng.invalidate_hnsw_cache("my_coll")
    assert not eng.hnsw_cache_contains("my_coll") and eng.hnsw_cache_keys("my_coll") is None


def test_cache_does_not_cross_collections(E):  # lib.rs:9909-9926
    eng = abc(E, ((1, 0, 0),))
    eng.build_and_cache_index()
    assert eng.hnsw_cache_contains(D)
    eng.cache_hnsw_index("other", empty_index(E), [])
    assert eng.hnsw_cache_contains("other")
    eng.invalidate_hnsw_cache(D)
    assert not eng.hnsw_cache_contains(D) and eng.hnsw_cache_contains("other")


def test_cache_empty_mapping_falls_through_to_brute_force(E):  # lib.rs:9929-9943
    eng = abc(E, ((1, 0, 0), (0, 1, 0)))
    eng.cache_hnsw_index(D, empty_index(E), [])
    res = eng.search_similar([1.0, 0.0, 0.0], 2)
    assert len(res) == 2 and res[0].key == "a"


# ---- parity on the golden corpus ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def golden():
    """(rows, queries, keys, the oracle's index over the rows in key order) — the oracle is built once for the module"""
    z = np.load(GOLDEN)
    rows, Q = z["rows"], z["queries"]
    m, m0, efc, efs, metric = z["config"].tolist()
    assert (m, m0, efc, efs, metric) == (16, 32, 200, 50, ho.COSINE)   # HNSWConfig::default, what build_and_cache_index(None) builds
    keys = [f"k{i:04d}" for i in range(len(rows))]
    return rows, Q, keys, ho.build(rows)


def golden_engine(E, golden):
    rows, Q, keys, o = golden
    eng = E.VectorEngine()
    eng.batch_store_embeddings(keys, rows)
    assert eng.list_keys() == keys
    return eng


def test_parity_with_the_cached_path_on_the_golden_corpus(E, golden):
    rows, Q, keys, o = golden
    eng = golden_engine(E, golden)
    eng.build_and_cache_index()
    assert eng.hnsw_cache_keys(D) == keys
    differs = 0
    for top_k in (1, 10, 60):
        for q in Q:
            got = eng.search_similar(q, top_k)
            assert pairs(got) == want_pairs(co.cached_search(o, keys, co.embedding_prefix(), q, top_k)), top_k
            er, es = oc.search(rows, q, top_k, 0)
            differs += [F(r.score).tobytes() for r in got] != [F(s).tobytes() for s in es]
    assert differs > 0      # the graph's scores: not the exhaustive cosine's bits
    eng.invalidate_hnsw_cache(D)
    for top_k in (1, 10, 60):
        for q in Q:
            er, es = oc.search(rows, q, top_k, 0)
            assert pairs(eng.search_similar(q, top_k)) == [(keys[int(r)], F(s).tobytes()) for r, s in zip(er, es)]


def test_inherited_callers_go_through_the_hook(E, golden):
    rows, Q, keys, o = golden
    eng = golden_engine(E, golden)
    eng.build_and_cache_index()
    # search_similar_paginated asks search_similar for total_needed(top_k, skip, limit) (lib.rs:2833-2858)
    page = eng.search_similar_paginated(Q[3], 10, E.Pagination(skip=4, limit=3))
    want = co.cached_search(o, keys, co.embedding_prefix(), Q[3], 7)[4:7]
    assert pairs(page.items) == want_pairs(want)


# ---- collections ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small():
    """(rows, queries, oracle index under Cosine): 120 x 12, a quarter duplicates"""
    rng = np.random.default_rng(0xCAC4E)
    rows = rng.standard_normal((120, 12)).astype(F)
    for i in range(4, 120, 4):
        rows[i] = rows[rng.integers(0, i)]
    return rows, rng.standard_normal((12, 12)).astype(F), ho.build(rows)


def scratch_index(E, rows, options=None):
    s = E.VectorEngine()
    keys = [f"r{i:03d}" for i in range(len(rows))]
    s.batch_store_embeddings(keys, rows)
    index, km = s.build_hnsw_index_with_options(options) if options else s.build_hnsw_index_default()
    assert km == keys
    return index, keys


def test_collection_metric_does_not_reach_the_cached_index(E, small):
    """a Euclidean collection cached with a Cosine index answers with the index's scores; storage-key and plain-key mappings; a
    mapping shorter than the index"""
    from neumann_amd import DistanceMetric
    rows, Q, o = small
    eng = E.VectorEngine()
    eng.create_collection("eu", E.VectorCollectionConfig().with_metric(DistanceMetric.Euclidean))
    for i, r in enumerate(rows):
        eng.store_in_collection("eu", f"r{i:03d}", r)
    brute = pairs(eng.search_in_collection("eu", Q[0], 5))
    index, keys = scratch_index(E, rows)
    prefix = co.collection_embedding_prefix("eu")
    for mapping in ([prefix + k for k in keys], keys, [prefix + k for k in keys[:50]], ["emb:" + k for k in keys]):
        eng.cache_hnsw_index("eu", index, mapping)
        for q in Q:
            got = eng.search_in_collection("eu", q, 8)
            assert pairs(got) == want_pairs(co.cached_search(o, mapping, prefix, q, 8))
    assert pairs(eng.search_in_collection("eu", Q[0], 5)) != brute
    eng.invalidate_hnsw_cache("eu")
    assert pairs(eng.search_in_collection("eu", Q[0], 5)) == brute
    # the zero-magnitude rule of the COLLECTION's metric stands in front of the hook (lib.rs:1617-1620): Euclidean lets a zero query in
    eng.cache_hnsw_index("eu", index, keys)
    zero = np.zeros(12, F)
    assert pairs(eng.search_in_collection("eu", zero, 3)) == want_pairs(co.cached_search(o, keys, prefix, zero, 3))
    eng.store_embedding("x", rows[0])
    eng.cache_hnsw_index(D, index, keys)
    assert eng.search_similar(zero, 3) == []                 # search_similar: zero magnitude answers [] before the hook (lib.rs:1970-1974)
    # a user collection named "_default" shares the default collection's entry, as in the reference
    eng.create_collection(D)
    eng.store_in_collection(D, "y", rows[1])                 # ... and so drops it (lib.rs:1497)
    assert not eng.hnsw_cache_contains(D)


# ---- the invalidation table -----------------------------------------------------------------------------------------------------
def test_invalidation_table(E, small, tmp_path):
    rows, Q, o = small
    index, keys = scratch_index(E, rows)
    eng = E.VectorEngine(E.VectorEngineConfig(max_dimension=12))
    eng.batch_store_embeddings(keys, rows)
    eng.create_collection("c", E.VectorCollectionConfig().with_dimension(12))
    eng.store_in_collection("c", "a", rows[0])

    def cached():
        eng.cache_hnsw_index(D, index, keys)
        eng.cache_hnsw_index("c", index, keys)
        return True

    def state():
        return eng.hnsw_cache_contains(D), eng.hnsw_cache_contains("c")

    # each of the four invalidates on success (lib.rs:1866, 1923, 1497, 1532), its own entry only ...
    assert cached() and eng.store_embedding("new", rows[1]) is None and state() == (False, True)
    assert cached() and eng.delete_embedding("new") is None and state() == (False, True)
    assert cached() and eng.store_in_collection("c", "b", rows[1]) is None and state() == (True, False)
    assert cached() and eng.store_in_collection_with_metadata("c", "b2", rows[2], {"t": 1}) is None and state() == (True, False)
    assert cached() and eng.delete_from_collection("c", "b") is None and state() == (True, False)
    # ... and not on failure
    cached()
    for call in (lambda: eng.store_embedding("bad", []), lambda: eng.store_embedding("bad", np.ones(13, F)),
                 lambda: eng.delete_embedding("missing"), lambda: eng.store_in_collection("c", "bad", np.ones(5, F)),
                 lambda: eng.delete_from_collection("c", "missing"), lambda: eng.delete_from_collection("nowhere", "a")):
        with pytest.raises(E.VectorError):
            call()
        assert state() == (True, True)
    # batch_store invalidates
    eng.batch_store_embeddings(["n1", "n2"], rows[:2])
    assert state() == (False, True)
    eng.batch_delete_embeddings(["n1", "n2"])
    # store_embedding_with_metadata, batch_delete, update_metadata, clear, delete_collection do not
    cached()
    eng.store_embedding_with_metadata("m", rows[3], {"tag": "x"})
    assert state() == (True, True)
    eng.update_metadata("m", {"tag": "y"})
    assert state() == (True, True)
    assert eng.batch_delete_embeddings([keys[7], "m"]) == 2
    assert state() == (True, True)
    # the stale answer names a deleted key
    got = eng.search_similar(rows[7], 3)
    assert pairs(got) == want_pairs(co.cached_search(o, keys, co.embedding_prefix(), rows[7], 3))
    assert keys[7] in [r.key for r in got] and not eng.exists(keys[7])
    eng.delete_collection("c")
    assert state() == (True, True)
    eng.clear()
    assert state() == (True, True) and eng.count() == 0
    assert pairs(eng.search_similar(rows[7], 3)) == pairs(got)
    # load_index: a named collection is restored through store_in_collection_with_metadata (lib.rs:3921-3929) and drops its entry;
    # the default collection through store_embedding_with_metadata, which drops nothing
    src = E.VectorEngine()
    src.store_embedding("d0", rows[0])
    src.create_collection("c")
    src.store_in_collection("c", "a", rows[0])
    src.save_index("default", str(tmp_path / "default.json"))
    src.save_index("c", str(tmp_path / "c.json"))
    cached()
    eng.load_index(str(tmp_path / "default.json"))
    assert state() == (True, True)
    eng.load_index(str(tmp_path / "c.json"))
    assert state() == (True, False)


# ---- fall-through rules, dimension mismatch ------------------------------------------------------------------------------------
def test_fall_through_and_dimension_rules(E, small):
    rows, Q, o = small
    index, keys = scratch_index(E, rows)
    eng = abc(E)
    brute = pairs(eng.search_similar([1.0, 0.0, 0.0], 2))
    eng.cache_hnsw_index(D, index, [])                       # an empty mapping falls through (even with a built index)
    assert pairs(eng.search_similar([1.0, 0.0, 0.0], 2)) == brute
    eng.cache_hnsw_index(D, empty_index(E), ["a", "b"])      # an empty index under a mapping answers [], with no fall-through
    assert eng.search_similar([1.0, 0.0, 0.0], 2) == []
    eng.cache_hnsw_index(D, index, keys)                     # re-caching replaces the entry
    with pytest.raises(E.VectorError) as e:
        eng.search_similar([1.0, 0.0, 0.0], 2)
    assert e.value.kind == "DimensionMismatch" and str(e.value) == "Dimension mismatch: expected 12, got 3"
    with pytest.raises(E.VectorError) as e:                  # the validations stand in front of the hook
        eng.search_similar(Q[0], 0)
    assert e.value.kind == "InvalidTopK"
    got = eng.search_similar(Q[0], 500)                      # top_k beyond the index: every node the walk reaches
    assert pairs(got) == want_pairs(co.cached_search(o, keys, co.embedding_prefix(), Q[0], 500))


# ---- handles and ownership -----------------------------------------------------------------------------------------------------
def test_the_cache_holds_its_own_reference(E, small, tmp_path):
    from neumann_amd import HNSWBuildOptions
    from tests import _hnsw_q8_oracle as q8
    rows, Q, o = small
    eng = abc(E)
    index, keys = scratch_index(E, rows)
    eng.cache_hnsw_index(D, index, keys)
    index.close()                                            # freeing the caller's handle leaves the cache answering
    want = [want_pairs(co.cached_search(o, keys, co.embedding_prefix(), q, 6)) for q in Q]
    assert [pairs(eng.search_similar(q, 6)) for q in Q] == want
    # a loaded handle
    index, keys = scratch_index(E, rows)
    eng.save_hnsw_index(index, str(tmp_path / "h.bin"))
    index.close()
    loaded, lkeys = eng.load_hnsw_index(str(tmp_path / "h.bin"))
    assert lkeys == keys
    eng.cache_hnsw_index("loaded", loaded)                   # the handle's own mapping
    loaded.close()
    eng.create_collection("loaded")
    assert [pairs(eng.search_in_collection("loaded", q, 6)) for q in Q] == want
    # a quantized handle
    qi, qkeys = scratch_index(E, rows, HNSWBuildOptions.memory_optimized())
    oq = q8.build(rows, ho.HNSWConfig.high_speed())
    eng.cache_hnsw_index(D, qi, qkeys)                       # replaces the dense entry
    qi.close()
    for q in Q:
        assert pairs(eng.search_similar(q, 6)) == want_pairs(co.cached_search(oq, qkeys, co.embedding_prefix(), q, 6))
    eng.close()                                              # nmn_engine_destroy drops the cache


# ---- concurrent engine callers -------------------------------------------------------------------------------------------------
def test_concurrent_engine_callers_receive_lone_answers(E, small):
    rows, Q, o = small
    eng = abc(E)
    index, keys = scratch_index(E, rows)
    eng.cache_hnsw_index(D, index, keys)
    jobs = [(Q[j % len(Q)], (1, 3, 10, 60, 200)[j % 5]) for j in range(16 * 12)]
    lone = [pairs(eng.search_similar(q, k)) for q, k in jobs]
    out = [None] * len(jobs)
    errs = []
    start = threading.Barrier(16)

    def work(t):
        try:
            start.wait()
            for j in range(t, len(jobs), 16):
                out[j] = pairs(eng.search_similar(*jobs[j]))
        except Exception as e:  # noqa: BLE001
            errs.append(e)

    th = [threading.Thread(target=work, args=(t,)) for t in range(16)]
    for x in th:
        x.start()
    for x in th:
        x.join()
    assert not errs, errs
    assert out == lone
    assert lone[3] == want_pairs(co.cached_search(o, keys, co.embedding_prefix(), *jobs[3]))
