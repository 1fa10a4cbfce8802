"""tests/_hnsw_mixed_oracle.py against answers derived by hand from the reference's text (docs/hnsw.md §15), the condition that makes
the GPU parity tests of tests/test_gpu_hnsw_mixed.py mean something, and the new symbols' declarations.  No GPU."""
import functools
import math
import os
import re

import numpy as np

from tests import _hnsw_mixed_oracle as mo
from tests import _hnsw_oracle as ho

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "hnsw_mixed_small.npz")
NEW_GPU_SYMBOLS = ["nmn_hnsw_insert_sparse", "nmn_hnsw_insert_auto", "nmn_hnsw_sparse_row"]
SV = mo.SparseVector


def bits(x):
    return np.asarray(x, dtype=F).reshape(-1).view(np.uint32).tolist()


def two_nodes(metric, a, b):
    """an index of two nodes, each ("s", SparseVector) or ("d", row)"""
    idx = mo.HNSWMixedIndex(ho.HNSWConfig().with_distance_metric(metric))
    for kind, v in (a, b):
        idx.insert_sparse(v) if kind == "s" else idx.insert(v)
    return idx


def query_distance(idx, node, q=None, sq=None):
    w = mo.HNSWMixedIndex.__new__(mo.HNSWMixedIndex)
    w.__dict__.update(idx.__dict__)
    w._sq = sq
    qd = sq.to_dense() if sq is not None else np.asarray(q, dtype=F)
    return w._dist_query([node], qd, w._qmag(qd))[0]


# ---- the query side ---------------------------------------------------------------------------------------------------------
def test_one_f64_chain_is_not_eight_f32_chains():
    """(0, 2^24), (1, 1), (2, -2^24) against ones: f64 keeps the 1.0 that f32 loses in 2^24 + 1"""
    big = 2.0 ** 24
    s = SV.from_parts(3, [0, 1, 2], [big, 1.0, -big])
    ones = np.ones(3, dtype=F)
    assert s.dot_dense(ones) == F(1.0)
    assert ho.dot_product_rows(s.to_dense()[None, :], ones)[0] == F(0.0)   # ((-0 + 2^24) + 1) + -2^24 in f32: the 1 is lost
    idx = two_nodes(ho.DOT_PRODUCT, ("s", s), ("d", s.to_dense()))
    assert bits(query_distance(idx, 0, q=ones)) == bits(F(-1.0))
    assert bits(query_distance(idx, 1, q=ones)) == bits(F(-0.0))


def test_a_node_without_entries():
    e = SV.from_parts(4, [], [])
    q = np.array([1, 2, 3, 4], dtype=F)
    Q = SV.from_dense(q)
    assert bits(e.dot_dense(q)) == bits(F(-0.0))            # Iterator::sum of nothing
    assert bits(e.dot(Q)) == bits(F(0.0))                   # dot_f64 starts at 0.0_f64
    assert math.copysign(1.0, e.magnitude_f64()) == -1.0 and e.magnitude() == 0.0   # sqrt(-0.0) = -0.0, == 0.0
    other = ("d", np.ones(4, dtype=F))
    cos = two_nodes(ho.COSINE, ("s", e), other)
    assert bits(query_distance(cos, 0, q=q)) == bits(F(1.0))
    assert bits(query_distance(cos, 0, sq=Q)) == bits(F(1.0))
    dot = two_nodes(ho.DOT_PRODUCT, ("s", e), other)
    assert bits(query_distance(dot, 0, q=q)) == bits(F(0.0))      # -(-0.0)
    assert bits(query_distance(dot, 0, sq=Q)) == bits(F(-0.0))    # -(+0.0)


def test_magnitude_goes_through_f64():
    s = SV.from_parts(2, [0, 1], [3e-30, 4e-30])
    assert ho.magnitude(s.to_dense()) == F(0.0)              # 9e-60 underflows in f32
    assert abs(float(s.magnitude()) / 5e-30 - 1.0) < 1e-6
    idx = two_nodes(ho.COSINE, ("s", s), ("d", s.to_dense()))
    q = np.array([1.0, 0.0], dtype=F)
    assert bits(query_distance(idx, 1, q=q)) == bits(F(1.0))       # the Dense node: a zero magnitude
    d = query_distance(idx, 0, q=q)                                # the Sparse node: 1 - 3e-30 / (5e-30 * 1)
    assert abs(float(d) - 0.4) < 1e-6


def test_duplicated_positions():
    s = SV.from_parts(3, [1, 1, 0], [2.0, 5.0, 1.0])
    assert s.positions == [0, 1, 1] and s.values.tolist() == [1.0, 2.0, 5.0]
    assert s.to_dense().tolist() == [1.0, 5.0, 0.0]                # the last of a position wins
    assert s.dot_dense(np.array([1, 1, 1], dtype=F)) == F(8.0)    # dot_dense counts both
    assert s.has_duplicates() and not SV.from_dense([1, 0, 2]).has_duplicates()
    t = SV.from_parts(3, [1], [10.0])
    assert s.dot(t) == F(20.0) and t.dot(s) == F(20.0)             # the merge pairs the first of the two only


def test_sparse_query_on_a_sparse_node():
    a = SV.from_parts(5, [0, 2, 4], [1.0, 2.0, 3.0])
    b = SV.from_parts(5, [2, 3, 4], [4.0, 5.0, 6.0])
    assert a.dot(b) == F(26.0)
    assert a.euclidean_distance(b) == F(math.sqrt(1 + 4 + 25 + 9))   # 1^2, (2-4)^2, (-5)^2, (3-6)^2
    idx = two_nodes(ho.EUCLIDEAN, ("s", a), ("d", b.to_dense()))
    assert bits(query_distance(idx, 0, sq=b)) == bits(F(math.sqrt(39.0)))
    huge = SV.from_parts(2, [0], [3e38])
    neg = SV.from_parts(2, [0], [-3e38])
    assert huge.euclidean_distance(neg) == F(np.finfo(F).max)          # the clamp


# ---- the pruning side: one pair per cell ----------------------------------------------------------------------------------------
def _pair_and_dense_twin(metric, a, b):
    """(the mixed arm, the Dense x Dense arm on to_dense()) for a pair of nodes"""
    idx = two_nodes(metric, a, b)
    twin = two_nodes(metric, ("d", idx.rows[0].copy()), ("d", idx.rows[1].copy()))
    return idx._dist_pairs(0, [1])[0], twin._dist_pairs(0, [1])[0]


BIG = 2.0 ** 24
S1 = SV.from_parts(3, [0, 1, 2], [BIG, 1.0, -BIG])
S_ONES = SV.from_parts(3, [0, 1, 2], [1.0, 1.0, 1.0])


def test_pruning_dot_product_cells():
    ss, dd = _pair_and_dense_twin(ho.DOT_PRODUCT, ("s", S1), ("s", S_ONES))
    assert bits(ss) == bits(F(-1.0)) and bits(dd) == bits(F(-0.0))
    ds, dd = _pair_and_dense_twin(ho.DOT_PRODUCT, ("d", np.ones(3, dtype=F)), ("s", S1))
    assert bits(ds) == bits(F(-1.0)) and bits(dd) == bits(F(-0.0))
    sd, _ = _pair_and_dense_twin(ho.DOT_PRODUCT, ("s", S1), ("d", np.ones(3, dtype=F)))
    assert bits(sd) == bits(ds)                                   # either order


def test_pruning_cosine_cells():
    tiny = SV.from_parts(2, [0, 1], [3e-30, 4e-30])
    unit = SV.from_parts(2, [0], [1.0])
    # S x S: magnitudes stay f64 — 3e-30 / (5e-30 * 1) = 0.6 -> 1 - 0.6f; the dense arm sees a zero magnitude
    ss, dd = _pair_and_dense_twin(ho.COSINE, ("s", tiny), ("s", unit))
    x3, x4 = float(F(3e-30)), float(F(4e-30))
    mag = math.sqrt(x3 * x3 + x4 * x4)
    assert bits(dd) == bits(F(1.0))
    assert bits(ss) == bits(F(1.0) - F(x3 / mag))
    # D x S: everything in f64, one cast
    ds, dd = _pair_and_dense_twin(ho.COSINE, ("d", np.array([1.0, 0.0], dtype=F)), ("s", tiny))
    assert bits(dd) == bits(F(1.0))
    assert bits(ds) == bits(F(1.0 - x3 / mag))
    # the two arms round differently: (1 - x) as f32 against 1f - (x as f32)
    x = SV.from_parts(3, [0, 1, 2], [1.0, 2.0, 3.0])
    y = np.array([3.0, 1.0, 2.0], dtype=F)
    r = 11.0 / (math.sqrt(14.0) * math.sqrt(14.0))
    ss, _ = _pair_and_dense_twin(ho.COSINE, ("s", x), ("s", SV.from_dense(y)))
    ds, _ = _pair_and_dense_twin(ho.COSINE, ("s", x), ("d", y))
    assert bits(ss) == bits(F(1.0) - F(r)) and bits(ds) == bits(F(1.0 - r))
    # zero magnitude: S x S gives 1 - 0 (similarity 0.0), D x S gives 1.0
    e = SV.from_parts(3, [], [])
    assert bits(_pair_and_dense_twin(ho.COSINE, ("s", e), ("s", x))[0]) == bits(F(1.0))
    assert bits(_pair_and_dense_twin(ho.COSINE, ("s", e), ("d", y))[0]) == bits(F(1.0))


def test_pruning_euclidean_cells():
    # S x S: 1 and eight times 2^-24.  In f32 every 1 + 2^-24 is a tie that rounds back to 1 (lanes 1 .. 7 and the scalar tail);
    # the f64 sum is 1 + 2^-21, whose root rounds to the f32 above 1
    a = SV.from_parts(9, [0], [1.0])
    b = SV.from_parts(9, list(range(1, 9)), [2.0 ** -12] * 8)
    ss, dd = _pair_and_dense_twin(ho.EUCLIDEAN, ("s", a), ("s", b))
    assert bits(ss) == bits(F(math.sqrt(1.0 + 2.0 ** -21))) and bits(dd) == bits(F(1.0)) and bits(ss) != bits(dd)
    # D x S is the D x D arm's own function on to_dense(): the exception
    ds, dd = _pair_and_dense_twin(ho.EUCLIDEAN, ("d", a.to_dense()), ("s", b))
    assert bits(ds) == bits(dd)


# ---- insert_auto ------------------------------------------------------------------------------------------------------------
def _kinds_after_auto(threshold, rows):
    """the kind insert_auto gives each row (an index of its own per row: a NaN row is scored against nothing)"""
    kinds = []
    for r in rows:
        idx = mo.HNSWMixedIndex(ho.HNSWConfig(sparsity_threshold=threshold))
        idx.insert_auto(r)
        kinds.append(idx.kind(0))
    return kinds


def test_insert_auto_threshold():
    half = np.array([1, 0, 2, 0], dtype=F)        # sparsity exactly 0.5
    quarter = np.array([1, 2, 3, 0], dtype=F)     # 0.25
    nan = np.array([np.nan, 0, 0, 0], dtype=F)    # NaN != 0.0: nnz 1, sparsity 0.75
    negz = np.array([-0.0, 0, 0, 0], dtype=F)     # -0.0 == 0.0: nnz 0, sparsity 1.0
    assert _kinds_after_auto(0.5, [half, quarter, nan, negz]) == ["sparse", "dense", "sparse", "sparse"]
    assert _kinds_after_auto(0.75, [half, nan]) == ["dense", "sparse"]
    assert _kinds_after_auto(0.0, [np.ones(4, dtype=F)]) == ["sparse"]
    assert _kinds_after_auto(1.0, [half, negz]) == ["dense", "sparse"]
    assert _kinds_after_auto(float("nan"), [half, negz]) == ["dense", "dense"]
    # f32: 1 - 7/10 is 0.3 rounded from the f32 quotient, compared with the f32 threshold
    r = np.zeros(10, dtype=F)
    r[:7] = 1
    sparsity = F(1.0) - F(7) / F(10)
    assert _kinds_after_auto(float(sparsity), [r]) == ["sparse"]
    assert _kinds_after_auto(float(np.nextafter(sparsity, F(1))), [r]) == ["dense"]
    idx = mo.HNSWMixedIndex(ho.HNSWConfig(sparsity_threshold=0.5))
    idx.insert_auto(np.array([-0.0, 5, 0, 0], dtype=F))
    assert bits(idx.rows[0]) == bits(np.array([0.0, 5, 0, 0], dtype=F))   # to_dense() of from_dense(): -0.0 is not stored
    assert idx.memory_stats() == {"total_nodes": 1, "dense_count": 0, "sparse_count": 1, "embedding_bytes": 56 + 8}


# ---- the condition of the GPU parity tests --------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _golden():
    return np.load(GOLDEN)


def test_golden_file_is_the_oracles():
    """the frozen file against the oracle of today, on a prefix (the whole build is the maker's, tests/golden/make_golden_hnsw_mixed.py)"""
    z = _golden()
    rows, mask, queries = mo.golden_corpus()
    assert np.array_equal(z["rows"].view(np.uint32), rows.view(np.uint32)) and np.array_equal(z["sparse_mask"], mask)
    assert np.array_equal(z["queries"].view(np.uint32), queries.view(np.uint32))
    n = 120
    idx = mo.build_mixed(rows[:n], mask[:n], ho.HNSWConfig().with_distance_metric(ho.DOT_PRODUCT))
    assert idx.levels == z["levels"][:n].tolist()       # the generator does not depend on the rows
    full_mask = z["sparse_mask"]
    assert [idx.kind(i) == "sparse" for i in range(n)] == full_mask[:n].tolist()


def test_mixed_answers_differ_from_the_all_dense_index():
    """64 queries, k 10, ef 50: how many get other ids or score bits from an all-dense index over the to_dense() rows — recorded
    by the maker from full oracle builds of both; at least 32 under DotProduct, at least 8 under Cosine"""
    z = _golden()
    for name, floor in (("dot", 32), ("cosine", 8)):
        mixed = (z[f"{name}_ids"], z[f"{name}_scores"].view(np.uint32))
        dense = (z[f"{name}_dense_ids"], z[f"{name}_dense_scores"].view(np.uint32))
        differ = int(((mixed[0] != dense[0]) | (mixed[1] != dense[1])).any(axis=1).sum())
        print(f"{name}: {differ} of {len(mixed[0])} queries differ from the all-dense index")
        assert differ == int(z[f"{name}_differ"]) and differ >= floor


# ---- declarations -------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_exported_declared_and_bound():
    from neumann_amd import _capi
    lib = _capi.load()
    gpu_h = open(os.path.join(ROOT, "include", "neumann_gpu.h")).read()
    ffi = open(os.path.join(ROOT, "integration", "rust", "ffi.rs")).read()
    wrapper = open(os.path.join(ROOT, "integration", "rust", "gpu_index.rs")).read()
    for name in NEW_GPU_SYMBOLS:
        assert hasattr(lib, name), name
        assert re.search(rf"\b{name}\s*\(", gpu_h), name
        assert re.search(rf"pub fn {name}\(", ffi), name
        assert name in _capi.SIGNATURES
        assert f"ffi::{name}" in wrapper, name
    from neumann_amd import GpuHnsw
    assert callable(GpuHnsw.insert_sparse) and callable(GpuHnsw.insert_auto) and callable(GpuHnsw.sparse_row)
