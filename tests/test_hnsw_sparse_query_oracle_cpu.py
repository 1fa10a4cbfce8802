"""tests/_hnsw_sparse_query_oracle.py held to known answers derived by hand (no GPU): the f64 chain of SparseVector::dot_dense
against the eight f32 chains of simd::dot_product, the order of the sum, the magnitude through f64, try_from_parts, the metrics
under which a sparse query IS the dense walk of its to_dense(), and the condition that keeps the GPU test from being vacuous."""
import functools
import os

import numpy as np
import pytest

from tests import _hnsw_oracle as ho
from tests import _hnsw_q8_oracle as q8
from tests import _hnsw_sparse_query_oracle as so
from tests import _xmetric_oracle as xo

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "hnsw_small_sparse.npz")


def bits(x):
    return np.ascontiguousarray(np.asarray(x, dtype=F)).view(np.uint32)


def test_f64_chain_against_f32_lanes():
    """2^24 + 1 - 2^24: exact in f64 (1.0); in f32 lane order -0.0 + 2^24 = 2^24, + 1 = 2^24 (tie to even), - 2^24 = 0.0"""
    sq = so.SparseQuery.from_parts(8, [0, 1, 2], [16777216.0, 1.0, -16777216.0])
    ones = np.ones(8, dtype=F)
    assert sq.dot_dense(ones) == F(1.0)
    assert ho.dot_product_rows(ones[None, :], sq.to_dense())[0] == F(0.0)


def test_the_sum_runs_in_position_order_whatever_the_input_order():
    """ascending: (2^24 + 1) + 2^-30 four times — each a quarter of an f64 ulp (2^-28), lost — = 16777217.0, a tie in f32, to even:
    16777216.0.  descending: 4 * 2^-30 = 2^-28, + 1, + 2^24 = 16777217 + 2^-28 exactly, above the tie: 16777218.0."""
    vals = [2.0 ** 24, 1.0, 2.0 ** -30, 2.0 ** -30, 2.0 ** -30, 2.0 ** -30]
    ones = np.ones(6, dtype=F)
    asc, desc = list(range(6)), list(range(5, -1, -1))
    assert so.SparseQuery.from_parts(6, asc, vals).dot_dense(ones) == F(16777216.0)
    assert so.SparseQuery.from_parts(6, desc, vals).dot_dense(ones) == F(16777218.0)
    perm = [3, 0, 5, 1, 4, 2]  # the same pairs, shuffled: try_from_parts sorts by position
    for pos in (asc, desc):
        want = so.SparseQuery.from_parts(6, pos, vals)
        got = so.SparseQuery.from_parts(6, [pos[i] for i in perm], [vals[i] for i in perm])
        assert got.positions == want.positions and bits(got.values).tolist() == bits(want.values).tolist()
        assert bits(got.dot_dense(ones)) == bits(want.dot_dense(ones))


def test_magnitude_goes_through_f64():
    """9e-60 + 16e-60 underflows to 0.0 in f32 and is an ordinary number in f64"""
    sq = so.SparseQuery.from_parts(4, [0, 1], [3e-30, 4e-30])
    mag = sq.magnitude()
    assert mag.dtype == F and mag == F(5e-30)
    dense = sq.to_dense()
    assert ho.magnitude(dense) == F(0.0)
    row = np.array([[1.0, 0.0, 0.0, 0.0]], dtype=F)
    o = ho.build(row, ho.HNSWConfig())
    (_, s_sparse), = so.search_sparse(o, sq, 1)
    (_, s_dense), = o.search(dense, 1)
    assert s_dense == F(0.0)                      # distance 1.0: the query's simd::magnitude is 0.0
    # dot = 3e-30 (f32), / (1.0 * 5e-30): similarity 0.6 up to the f32 roundings of the three values
    assert abs(float(s_sparse) - 0.6) < 1e-6


def test_from_parts():
    sq = so.SparseQuery.from_parts(5, [4, 2, 2, 0, 3, 2], [1.0, 7.0, 0.0, -0.0, np.nan, 9.0])
    assert sq.positions == [2, 2, 3, 4]           # zeros of either sign dropped, NaN kept, duplicates in input order
    assert sq.values[0] == 7.0 and sq.values[1] == 9.0 and np.isnan(sq.values[2]) and sq.values[3] == 1.0
    d = sq.to_dense()
    assert d[2] == 9.0 and d[0] == 0.0 and d[4] == 1.0  # the last of a duplicated position wins
    dup = so.SparseQuery.from_parts(3, [1, 1], [2.0, 3.0])
    assert dup.dot_dense(np.array([0, 10, 0], dtype=F)) == F(50.0)             # dot_dense counts BOTH entries
    assert dup.magnitude() == F(np.sqrt(13.0))
    with pytest.raises(so.IndexOutOfBounds, match="index 5 out of bounds for dimension 5"):
        so.SparseQuery.from_parts(5, [0, 5], [1.0, 1.0])
    with pytest.raises(so.IndexOutOfBounds):
        so.SparseQuery.from_parts(5, [5], [0.0])  # the position is checked before the zero is dropped
    empty = so.SparseQuery.from_parts(4, [1, 3], [0.0, -0.0])
    assert len(empty) == 0
    dot = empty.dot_dense(np.ones(4, dtype=F))
    assert dot == 0.0 and np.signbit(dot)         # the fold starts at -0.0
    assert empty.magnitude() == F(0.0)
    fd = so.SparseQuery.from_dense([0.0, 2.0, -0.0, np.nan])
    assert fd.positions == [1, 3] and fd.dimension == 4
    o = ho.build(np.eye(4, dtype=F), ho.HNSWConfig())
    assert all(s == F(0.0) for _, s in so.search_sparse(o, empty, 4))          # Cosine: every distance 1.0
    o = ho.build(np.eye(4, dtype=F), ho.HNSWConfig().with_distance_metric(ho.DOT_PRODUCT))
    res = so.search_sparse(o, empty, 4)
    assert all(s == 0.0 and np.signbit(s) for _, s in res)                     # distance -(-0.0) = +0.0, similarity -(+0.0)


@functools.lru_cache(maxsize=None)
def small(storage, metric):
    rng = np.random.default_rng(77)
    rows = rng.standard_normal((150, 12)).astype(F)
    rows[rng.random(rows.shape) < 0.5] = 0.0
    cfg = ho.HNSWConfig.high_speed().with_distance_metric(metric)
    return (q8.build if storage == "quantized" else ho.build)(rows, cfg)


def small_queries():
    rng = np.random.default_rng(78)
    Q = rng.standard_normal((12, 12)).astype(F)
    Q[rng.random(Q.shape) < 0.7] = 0.0
    return Q


@pytest.mark.parametrize("storage,metric", [("dense", ho.EUCLIDEAN), ("quantized", ho.EUCLIDEAN), ("quantized", ho.DOT_PRODUCT)])
def test_identities_with_the_dense_walk(storage, metric):
    o = small(storage, metric)
    for q in small_queries():
        sq = so.SparseQuery.from_dense(q)
        got = so.search_sparse_with_ef(o, sq, 10, 30)
        want = o.search_with_ef(sq.to_dense(), 10, 30)
        assert [i for i, _ in got] == [i for i, _ in want]
        assert bits([s for _, s in got]).tolist() == bits([s for _, s in want]).tolist()


def test_quantized_cosine_differs_only_through_the_query_magnitude():
    o = small("quantized", ho.COSINE)
    for q in small_queries():
        sq = so.SparseQuery.from_dense(q)
        ids = np.arange(o.n)
        d_sparse = so._walker(o, sq)._dist_query(ids, sq.to_dense(), sq.magnitude())
        d_dense_with_sparse_mag = o._dist_query(ids, sq.to_dense(), sq.magnitude())
        assert bits(d_sparse).tolist() == bits(d_dense_with_sparse_mag).tolist()
        w = so._walker(o, sq)
        assert w._qmag(sq.to_dense()) == sq.magnitude()


def test_golden_corpus_sparse_scores_differ_from_dense_scores():
    """what makes the GPU test able to tell the sparse walk from a densifying shortcut: under Cosine at least half the queries
    of the golden corpus get score bits from the sparse walk that the dense walk of to_dense(q) does not give"""
    o = xo.index_from_golden(GOLDEN)
    _, queries = xo.sparse_golden_corpus()
    differ = same_ids = 0
    for q in queries:
        sq = so.SparseQuery.from_dense(q)
        got = so.search_sparse_with_ef(o, sq, 10, 50)
        want = o.search_with_ef(q, 10, 50)
        same_ids += [i for i, _ in got] == [i for i, _ in want]
        differ += bits([s for _, s in got]).tolist() != bits([s for _, s in want]).tolist()
    print(f"golden corpus, Cosine, k 10, ef 50: {differ} of {len(queries)} queries differ in score bits, {same_ids} have equal ids")
    assert differ >= 32
