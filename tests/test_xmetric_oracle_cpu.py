"""The extended-metric oracle (tests/_xmetric_oracle.py) against the reference's own unit expectations, restated as literals, and
the host-only faces of the library (to_similarity, higher_is_better, the GeometricConfig presets, the exported symbols)."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

from neumann_amd import _capi
from oracle import oracle_c as oc
from tests import _hnsw_oracle as ho
from tests import _xmetric_oracle as xo

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M = xo.Metric
SV = xo.Sparse


def comp(kind, a, b, cfg=None):
    return float(xo.compute(M(kind, cfg), SV(a), SV(b)))


# ---- tensor_store/src/distance.rs:196 ff. -----------------------------------------------------------------------------------
def test_distance_rs_unit_expectations():
    assert xo.higher_is_better(M(xo.COSINE)) and xo.higher_is_better(M(xo.JACCARD))
    assert xo.higher_is_better(M(xo.OVERLAP)) and xo.higher_is_better(M(xo.WEIGHTED_JACCARD))
    assert xo.higher_is_better(M(xo.COMPOSITE, xo.GeometricConfig.default()))
    for k in (xo.ANGULAR, xo.GEODESIC, xo.EUCLIDEAN, xo.MANHATTAN):
        assert not xo.higher_is_better(M(k))
    assert abs(comp(xo.COSINE, [1.0, 0.0], [1.0, 0.0]) - 1.0) < 1e-6
    assert abs(comp(xo.JACCARD, [1.0, 0.0, 2.0], [3.0, 0.0, 4.0]) - 1.0) < 1e-6
    ts = lambda k, raw, cfg=None: float(xo.to_similarity(M(k, cfg), F(raw)))
    assert abs(ts(xo.COSINE, 1.0) - 1.0) < 1e-6 and abs(ts(xo.COSINE, -1.0)) < 1e-6 and abs(ts(xo.COSINE, 0.0) - 0.5) < 1e-6
    assert abs(ts(xo.ANGULAR, 0.0) - 1.0) < 1e-6 and abs(ts(xo.ANGULAR, xo.PI32)) < 1e-6
    assert abs(ts(xo.EUCLIDEAN, 0.0) - 1.0) < 1e-6 and abs(ts(xo.EUCLIDEAN, 1.0) - 0.5) < 1e-6
    assert abs(comp(xo.COMPOSITE, [1.0, 2.0, 3.0], [1.0, 2.0, 3.0], xo.GeometricConfig.default()) - 1.0) < 1e-6
    a, b = [1.0, 0.0], [0.0, 1.0]
    assert comp(xo.COMPOSITE, a, b, xo.GeometricConfig.angular_heavy()) < 0.5
    assert comp(xo.COMPOSITE, a, b, xo.GeometricConfig.structural_heavy()) < 0.5
    cd = xo.GeometricConfig.conflict_detection()
    assert cd.structural_weight > cd.cosine_weight and cd.structural_weight > cd.magnitude_weight
    assert abs(comp(xo.ANGULAR, [1.0, 0.0], [1.0, 0.0])) < 1e-5
    assert abs(comp(xo.GEODESIC, [1.0, 0.0], [1.0, 0.0])) < 1e-5
    assert abs(comp(xo.OVERLAP, [1.0, 0.0, 2.0], [3.0, 0.0, 4.0]) - 1.0) < 1e-6
    assert abs(comp(xo.WEIGHTED_JACCARD, [1.0, 2.0, 3.0], [1.0, 2.0, 3.0]) - 1.0) < 1e-6
    assert abs(comp(xo.EUCLIDEAN, [0.0, 0.0], [3.0, 4.0]) - 5.0) < 1e-6
    assert abs(comp(xo.MANHATTAN, [0.0, 0.0], [3.0, 4.0]) - 7.0) < 1e-6
    assert abs(comp(xo.COMPOSITE, [1.0, 2.0], [1.0, 2.0], xo.GeometricConfig.default()) - 1.0) < 1e-6
    assert abs(ts(xo.JACCARD, 0.5) - 0.5) < 1e-6 and abs(ts(xo.JACCARD, 1.0) - 1.0) < 1e-6
    assert abs(ts(xo.OVERLAP, 0.75) - 0.75) < 1e-6
    assert abs(ts(xo.WEIGHTED_JACCARD, 0.8) - 0.8) < 1e-6
    assert abs(ts(xo.COMPOSITE, 0.6, xo.GeometricConfig.default()) - 0.6) < 1e-6
    assert abs(ts(xo.GEODESIC, 0.0) - 1.0) < 1e-6
    assert abs(ts(xo.MANHATTAN, 0.0) - 1.0) < 1e-6 and abs(ts(xo.MANHATTAN, 1.0) - 0.5) < 1e-6
    assert comp(xo.COMPOSITE, [1.0, 2.0], [1.0, 2.0], xo.GeometricConfig(0.0, 0.0, 0.0)) == 0.0


# ---- tensor_store/src/sparse_vector.rs:1574-1773 ----------------------------------------------------------------------------
def test_sparse_vector_rs_metric_expectations():
    assert abs(comp(xo.ANGULAR, [1.0, 2.0, 3.0], [1.0, 2.0, 3.0])) < 1e-3
    assert abs(comp(xo.ANGULAR, [1.0, 0.0], [0.0, 1.0]) - math.pi / 2) < 1e-6
    assert abs(comp(xo.ANGULAR, [1.0, 0.0], [-1.0, 0.0]) - float(xo.PI32)) < 1e-6
    assert abs(comp(xo.JACCARD, [1.0, 0.0, 2.0, 0.0], [3.0, 0.0, 4.0, 0.0]) - 1.0) < 1e-6
    assert abs(comp(xo.JACCARD, [1.0, 0.0, 0.0, 0.0], [0.0, 0.0, 2.0, 0.0])) < 1e-6
    assert abs(comp(xo.JACCARD, [1.0, 2.0, 0.0, 0.0], [0.0, 3.0, 4.0, 0.0]) - 1.0 / 3.0) < 1e-6
    assert abs(comp(xo.OVERLAP, [0.0, 1.0, 0.0], [1.0, 2.0, 3.0]) - 1.0) < 1e-6
    assert abs(comp(xo.WEIGHTED_JACCARD, [1.0, 2.0, 3.0], [1.0, 2.0, 3.0]) - 1.0) < 1e-6
    assert abs(comp(xo.WEIGHTED_JACCARD, [1.0, 0.0], [2.0, 0.0]) - 0.5) < 1e-6
    assert abs(comp(xo.EUCLIDEAN, [1.0, 0.0], [0.0, 1.0]) - float(np.sqrt(F(2.0)))) < 1e-6
    assert abs(comp(xo.MANHATTAN, [1.0, 0.0, 3.0], [0.0, 2.0, 1.0]) - 5.0) < 1e-6
    assert abs(comp(xo.ANGULAR, [1.0, 0.0], [0.707, 0.707]) - comp(xo.GEODESIC, [1.0, 0.0], [0.707, 0.707])) < 1e-6
    assert 0.0 <= comp(xo.WEIGHTED_JACCARD, [1.0, 0.0, 3.0, 0.0], [0.0, 2.0, 4.0, 0.0]) <= 1.0
    assert 0.0 <= comp(xo.WEIGHTED_JACCARD, [1.0, 2.0, 3.0, 4.0], [1.0, 0.0, 0.0, 0.0]) <= 1.0
    assert abs(comp(xo.EUCLIDEAN, [1.0, 0.0, 2.0, 0.0], [0.0, 3.0, 0.0, 4.0]) - float(np.sqrt(F(30.0)))) < 1e-5
    assert abs(comp(xo.EUCLIDEAN, [1.0, 2.0, 3.0, 4.0], [1.0, 0.0, 0.0, 0.0]) - float(np.sqrt(F(29.0)))) < 1e-5
    assert abs(comp(xo.EUCLIDEAN, [1.0, 0.0, 0.0, 0.0], [1.0, 2.0, 3.0, 4.0]) - float(np.sqrt(F(29.0)))) < 1e-5
    assert abs(comp(xo.MANHATTAN, [1.0, 0.0, 2.0, 0.0], [0.0, 3.0, 0.0, 4.0]) - 10.0) < 1e-6


def test_from_dense_and_the_f32_steps():
    s = SV(np.array([0.0, -0.0, 1.5, np.nan, 0.0], dtype=F))
    assert s.positions == [2, 3] and s.values[0] == 1.5 and math.isnan(s.values[1])
    # midpoint and mul_add round once
    assert xo.midpoint(F(1.0), F(1.0)) == F(1.0) and xo.midpoint(F(-1.0), F(1.0)) == F(0.0)
    a, b, c = F(1.0 + 2.0 ** -23), F(1.0 + 2.0 ** -23), F(-(1.0 + 2.0 ** -22))
    assert float(xo.mul_add(a, b, c)) == 2.0 ** -46          # the product's low bits survive the fused add
    assert float(F(F(a * b) + c)) == 0.0
    assert np.signbit(xo.mul_add(F(-0.0), F(1.0), F(-0.0))) and not np.signbit(xo.mul_add(F(1.0), F(1.0), F(-1.0)))
    # the clamp of euclidean / manhattan at f32::MAX
    big = np.full(4, 3e38, dtype=F)
    assert comp(xo.EUCLIDEAN, big, np.zeros(4, dtype=F)) == xo.F32_MAX
    assert comp(xo.MANHATTAN, big, -big) == xo.F32_MAX


# ---- vector_engine/src/lib.rs:5455-5536, 5853-5944 --------------------------------------------------------------------------
def create_test_vector(dim, seed):  # tests::create_test_vector (lib.rs:4029-4038)
    i = np.arange(dim, dtype=np.int64)
    x = (seed * 31 + i * 17).astype(F)
    return (np.sin(x * F(0.0001), dtype=F) * ((seed + i).astype(F) * F(0.001))).astype(F)


def engine_case(named, query, top_k, kind):
    keys = [k for k, _ in named]
    vecs = {k: np.asarray(v, dtype=F) for k, v in named}
    idx = ho.build(np.stack([vecs[k] for k in keys]))
    return xo.search_with_hnsw_and_metric(idx, keys, vecs, np.asarray(query, dtype=F), top_k, M(kind))


def test_engine_expectations_of_the_reference():
    named = [(f"v{i}", create_test_vector(32, i)) for i in range(50)]
    res = engine_case(named, create_test_vector(32, 25), 5, xo.COSINE)
    assert len(res) == 5 and any(k == "v25" for k, _ in res)
    res = engine_case([("a", [1.0, 0.0]), ("b", [2.0, 0.0]), ("c", [10.0, 0.0])], [1.0, 0.0], 3, xo.EUCLIDEAN)
    assert len(res) == 3 and res[0][0] == "a"
    res = engine_case([("a", [1.0, 0.0]), ("b", [0.707, 0.707]), ("c", [0.0, 1.0])], [1.0, 0.0], 3, xo.ANGULAR)
    assert len(res) == 3 and res[0][0] == "a"
    res = engine_case([("a", [1.0, 1.0, 0.0]), ("b", [1.0, 0.0, 0.0]), ("c", [0.0, 0.0, 1.0])], [1.0, 1.0, 0.0], 3, xo.JACCARD)
    assert len(res) == 3 and res[0][0] == "a"
    res = engine_case([("a", [1.0, 1.0, 0.0]), ("b", [1.0, 0.0, 0.0])], [1.0, 1.0, 0.0], 2, xo.OVERLAP)
    assert len(res) == 2
    res = engine_case([("origin", [0.0, 0.0]), ("one", [1.0, 0.0]), ("two", [2.0, 0.0])], [0.0, 0.0], 3, xo.MANHATTAN)
    assert len(res) == 3 and res[0][0] == "origin"
    empty = ho.HNSWIndex()
    with pytest.raises(ValueError, match="Empty vector"):
        xo.search_with_hnsw_and_metric(empty, [], {}, [], 5, M(xo.COSINE))
    with pytest.raises(ValueError, match="Invalid top_k"):
        xo.search_with_hnsw_and_metric(empty, [], {}, [1.0], 0, M(xo.COSINE))
    assert xo.search_with_hnsw_and_metric(empty, [], {}, [1.0], 3, M(xo.COSINE)) == []
    assert xo.candidate_count(1) == 10 and xo.candidate_count(5) == 10 and xo.candidate_count(10) == 20
    assert xo.candidate_count((1 << 64) - 1) == (1 << 64) - 1


def test_gone_keys_short_mappings_and_current_vectors():
    rng = np.random.default_rng(3)
    rows = rng.standard_normal((40, 6)).astype(F)
    keys = [f"k{i}" for i in range(40)]
    idx = ho.build(rows)
    cur = {k: rows[i] for i, k in enumerate(keys)}
    q = rows[7]
    full = xo.search_with_hnsw_and_metric(idx, keys, cur, q, 5, M(xo.EUCLIDEAN))
    assert full[0][0] == "k7" and float(full[0][1]) == 1.0
    del cur["k7"]
    gone = xo.search_with_hnsw_and_metric(idx, keys, cur, q, 5, M(xo.EUCLIDEAN))
    assert all(k != "k7" for k, _ in gone) and gone[:4] == full[1:5]
    short = xo.search_with_hnsw_and_metric(idx, keys[:20], cur, q, 10, M(xo.EUCLIDEAN))
    assert all(int(k[1:]) < 20 for k, _ in short)
    cur[full[1][0]] = np.zeros(3, dtype=F)  # a current vector of another length: zero-padded by the merge
    moved = dict(xo.search_with_hnsw_and_metric(idx, keys, cur, q, 10, M(xo.EUCLIDEAN)))
    assert moved[full[1][0]] == xo.score_dense(M(xo.EUCLIDEAN), q, np.zeros(6, dtype=F))[1]


# ---- the oracle's Cosine against oracle/'s sparse_cos64 ----------------------------------------------------------------------
def test_cosine_matches_the_c_oracle_bit_for_bit():
    rng = np.random.default_rng(11)
    for dim in (1, 7, 8, 9, 37, 200):
        A = rng.standard_normal((12, dim)).astype(F)
        B = rng.standard_normal((12, dim)).astype(F)
        B[rng.random(B.shape) < 0.6] = 0.0
        A[3] = 0.0
        A[4] *= F(1e30)
        B[5] *= F(1e-30)
        B[6, 0] = -0.0
        for a in A:
            for b in B:
                want = oc.sparse_cos64(a, b)
                got = xo.cosine_similarity(SV(a), SV(b))
                assert got.tobytes() == want.tobytes(), (dim, a, b)


# ---- the library's host-only faces -------------------------------------------------------------------------------------------
def xm(kind, cfg=None):
    w = cfg.weights() if cfg else (0.0, 0.0, 0.0)
    return _capi.XMetric(kind, *[float(x) for x in w])


def test_library_to_similarity_and_higher_is_better_match_the_oracle():
    lib = _capi.load()
    raws = [0.0, -0.0, 1.0, -1.0, 0.5, 0.3333333, 3.1415927, 1.5707964, 1e-30, 3.4028235e38, 2.5, 1e-45, 0.99999994]
    for kind in range(9):
        cfg = xo.GeometricConfig.default() if kind == xo.COMPOSITE else None
        m = xm(kind, cfg)
        assert bool(lib.nmn_xmetric_higher_is_better(C.byref(m))) == xo.higher_is_better(M(kind, cfg))
        for raw in raws:
            got = F(lib.nmn_xmetric_to_similarity(C.byref(m), float(F(raw))))
            want = xo.to_similarity(M(kind, cfg), F(raw))
            assert got.tobytes() == want.tobytes(), (kind, raw, got, want)
    bad = _capi.XMetric(9, 0.0, 0.0, 0.0)
    assert math.isnan(lib.nmn_xmetric_to_similarity(C.byref(bad), 0.5))


def test_geometric_presets_match_the_reference():
    from neumann_amd import ExtendedDistanceMetric, GeometricConfig
    for name in ("default", "angular_heavy", "structural_heavy", "conflict_detection"):
        got = getattr(GeometricConfig, name)()
        want = getattr(xo.GeometricConfig, name)()
        assert (F(got.cosine_weight), F(got.structural_weight), F(got.magnitude_weight)) == want.weights(), name
    names = [n for n in ExtendedDistanceMetric._NAMES]
    assert names == list(xo.NAMES)
    assert ExtendedDistanceMetric.WeightedJaccard.kind == xo.WEIGHTED_JACCARD
    c = ExtendedDistanceMetric.Composite(GeometricConfig.structural_heavy())
    assert c.kind == xo.COMPOSITE and c.higher_is_better() and not ExtendedDistanceMetric.Manhattan.higher_is_better()
    assert ExtendedDistanceMetric.Cosine.to_similarity(0.0) == 0.5


def test_every_new_symbol_is_declared_and_exported():
    lib = _capi.load()
    hdr = open(os.path.join(ROOT, "include", "neumann_gpu.h")).read()
    for n in ("nmn_xmetric_geometric_default", "nmn_xmetric_geometric_angular_heavy", "nmn_xmetric_geometric_structural_heavy",
              "nmn_xmetric_geometric_conflict_detection", "nmn_xmetric_to_similarity", "nmn_xmetric_higher_is_better",
              "nmn_index_score_rows_xmetric", "nmn_xmetric_score_host_rows", "nmn_hnsw_search_metric",
              "nmn_hnsw_search_metric_device"):
        assert re.search(rf"\b{n}\s*\(", hdr), n
        assert hasattr(lib, n), n
    eng = open(os.path.join(ROOT, "include", "neumann_engine.h")).read()
    assert re.search(r"\bnmn_engine_search_with_hnsw_and_metric\s*\(", eng)
    assert re.search(r"\bnmn_engine_search_with_hnsw_and_metric_mapped\s*\(", eng)
    assert hasattr(lib, "nmn_engine_search_with_hnsw_and_metric") and hasattr(lib, "nmn_engine_search_with_hnsw_and_metric_mapped")
    for i, name in enumerate(("COSINE", "ANGULAR", "GEODESIC", "JACCARD", "OVERLAP", "WEIGHTED_JACCARD", "EUCLIDEAN", "MANHATTAN",
                              "COMPOSITE")):
        assert re.search(rf"#define NMN_XMETRIC_{name} {i}\b", hdr), name
        assert getattr(_capi, "XMETRIC_" + name) == i


def test_sparse_golden_file_is_the_oracles_corpus():
    """tests/golden/hnsw_small_sparse.npz (make_golden_hnsw_sparse.py): the rows it was built over are sparse_golden_corpus(), the
    graph is well formed, and walking it gives what the stored rows say (the build itself is not repeated here: ten seconds)"""
    path = os.path.join(ROOT, "tests", "golden", "hnsw_small_sparse.npz")
    g = np.load(path)
    rows, queries = xo.sparse_golden_corpus()
    assert np.array_equal(g["rows"], rows) and np.array_equal(g["queries"], queries)
    assert g["config"].tolist() == [16, 32, 200, 50, ho.COSINE]
    assert 0.55 < float(np.mean(rows == 0.0)) < 0.65
    idx = xo.index_from_golden(path)
    assert len(idx) == 800 and idx.levels[idx.entry_point] == idx.max_layer
    for node, per_layer in enumerate(idx.neighbors):
        for layer, lst in enumerate(per_layer):
            assert lst == sorted(lst) and node not in lst and len(lst) <= (32 if layer == 0 else 16)
            assert all(idx.levels[n] >= layer for n in lst)
    # the first 60 nodes rebuilt from scratch take the same levels (the generator's sequence) as the file records
    small = ho.build(rows[:60])
    assert small.levels == idx.levels[:60]
    assert os.path.getsize(path) < 1 << 20
