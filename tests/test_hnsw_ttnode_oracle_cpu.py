"""tests/_hnsw_ttnode_oracle.py against hand-derived values — one per rule by which an EmbeddingStorage::TensorTrain node is scored
(docs/hnsw.md §24) — the new symbols, and the frozen fixture tests/golden/hnsw_ttnode_small.npz.  No GPU.  (The library's host
walk is held to the twin in tests/test_gpu_hnsw_ttnode.py: a handle cannot be created without a device.)"""
import os
import re

import numpy as np
import pytest

from tests import _hnsw_mixed_oracle as mo
from tests import _hnsw_oracle as ho
from tests import _hnsw_tt_oracle as to
from tests import _hnsw_ttnode_oracle as tn
from tests import _tt_similarity_oracle as so

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "hnsw_ttnode_small.npz")
METRICS = [ho.COSINE, ho.EUCLIDEAN, ho.DOT_PRODUCT]


def bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


def fbits(u):
    return np.array([u], dtype=np.uint32).view(F)[0]


def cfg(metric):
    return ho.HNSWConfig.high_speed().with_distance_metric(metric)


def single(x, shape=(2, 2, 5)):
    """a rank-one train whose reconstruction is x at element 0 and zeros elsewhere; tt_norm = sqrt(x * x)"""
    cores = [np.zeros(n, dtype=F) for n in shape]
    for c in cores:
        c[0] = 1.0
    cores[0][0] = x
    return to.TTVector(list(shape), [1] * (len(shape) + 1), cores)


def unit(dim, at=0):
    v = np.zeros(dim, dtype=F)
    v[at] = 1.0
    return v


# ---- rule 1: a dense or sparse query divides by the CACHED norm --------------------------------------------------------------------
def test_rule1_dense_query_divides_by_the_cached_norm_not_simd_magnitude():
    """[4096, 1, ..., 1] of 16 elements as ONE core (§17's example): tt_norm's single chain stays at 2^24, 4096.0 = 0x45800000;
    simd::magnitude keeps eight chains and gives sqrt(2^24 + 14) = 0x45800003.  The query is the row itself: dot = 2^24 + 14,
    mag_query = 0x45800003.  The TT node divides by 4096 * mag_query, the Dense node by mag_query^2."""
    v = np.ones(16, dtype=F)
    v[0] = 4096.0
    tt = to.TTVector([16], [1, 1], [v])
    assert bits(to.tt_norm(tt)) == 0x45800000 and bits(ho.magnitude(v)) == 0x45800003
    dot, mq = F(2 ** 24 + 14), fbits(0x45800003)
    assert bits(ho.dot_product_rows(v[None, :], v)[0]) == bits(dot)
    want_tt = F(1.0) - dot / (F(4096.0) * mq)
    want_dense = F(1.0) - dot / (mq * mq)
    assert bits(want_tt) != bits(want_dense)
    t = tn.build([("tt", tt)], cfg(ho.COSINE))
    d = tn.build([("dense", v)], cfg(ho.COSINE))
    assert t.kind(0) == "tt" and d.kind(0) == "dense"
    assert np.array_equal(bits(t.rows[0]), bits(v))                       # the row of a TT node is its reconstruction
    (_, st), = t.search_with_ef(v, 1, 10)
    (_, sd), = d.search_with_ef(v, 1, 10)
    assert bits(st) == bits(F(1.0) - want_tt) and bits(sd) == bits(F(1.0) - want_dense)
    # a sparse query: dot_dense through f64 over the stored entries, the same cached norm (1069-1079)
    sq = mo.SparseVector.from_dense(unit(16))
    (_, ss), = t.search_sparse_with_ef(sq, 1, 10)
    assert bits(ss) == bits(F(1.0) - (F(1.0) - F(4096.0) / (F(4096.0) * F(1.0)))) and ss == 1.0
    (_, sds), = d.search_sparse_with_ef(sq, 1, 10)
    assert bits(sds) == bits(F(1.0) - (F(1.0) - F(4096.0) / (mq * F(1.0)))) and sds != 1.0
    # Euclidean and DotProduct: the Dense arithmetic on the reconstruction, no magnitude read
    for metric in (ho.EUCLIDEAN, ho.DOT_PRODUCT):
        a = tn.build([("tt", tt)], cfg(metric)).search_with_ef(unit(16, 3), 1, 10)
        b = tn.build([("dense", v)], cfg(metric)).search_with_ef(unit(16, 3), 1, 10)
        assert a[0][0] == b[0][0] and bits(a[0][1]) == bits(b[0][1])


def test_a_tiny_norm_is_a_real_quotient_for_a_dense_query_and_1_for_a_tt_query():
    """node norm 5e-11 (below 1e-10, not 0.0).  Dense query e0: dot = x, mag_self = x, mag_query = 1: 1 - x / (x * 1) = 0.0, a real
    quotient — `== 0.0` does not fire.  TT query: `cached.norm < 1e-10` fires: 1.0.  T x T pruning: 1.0.  T x D pruning divides by
    simd::magnitude(reconstruction) = sqrt(x * x) = x, not 0: 1 - x / (x * 1) = 0.0."""
    x = F(5e-11)
    node = single(x)
    assert bits(to.tt_norm(node)) == bits(x) and x < tn.TINY and x != 0
    idx = tn.build([("tt", node), ("tt", single(F(2.0))), ("dense", unit(20))], cfg(ho.COSINE))
    assert bits(idx._dist_query([0], unit(20), F(1.0))[0]) == bits(F(0.0))
    q = single(F(1.0))
    assert idx.tt_node_distance(0, q, to.tt_norm(q)) == 1.0
    assert idx.tt_node_distance(1, q, to.tt_norm(q)) == 0.0               # 1 - 2 / (2 * 1)
    assert idx._dist_pairs(0, [1])[0] == 1.0 and idx._dist_pairs(1, [0])[0] == 1.0
    assert bits(idx.mags[0]) == bits(x)
    assert bits(idx._dist_pairs(0, [2])[0]) == bits(F(0.0)) and bits(idx._dist_pairs(2, [0])[0]) == bits(F(0.0))


def test_node_norms_just_below_at_and_just_above_the_threshold():
    tiny = F(1e-10)
    below, above = np.nextafter(tiny, F(0)), np.nextafter(tiny, F(1))
    idx = tn.build([("tt", single(x)) for x in (below, tiny, above)], cfg(ho.COSINE))
    assert [bits(idx.tt[i][1]).item() for i in range(3)] == [bits(x).item() for x in (below, tiny, above)]
    q = single(F(1.0))
    d = idx.cosine_distance_tt_with_norm([0, 1, 2], q, to.tt_reconstruct(q), to.tt_norm(q))
    assert d.tolist() == [1.0, 0.0, 0.0]                                  # `<`: at the threshold the arithmetic runs, x / (x * 1)
    # the same three as QUERY norms against a node of norm 1 (the first test of the function)
    one = tn.build([("tt", single(F(1.0)))], cfg(ho.COSINE))
    got = [one.tt_node_distance(0, single(x), to.tt_norm(single(x))) for x in (below, tiny, above)]
    assert got == [1.0, 0.0, 0.0]
    # pruning T x T: either norm below
    assert idx._dist_pairs(0, [1, 2]).tolist() == [1.0, 1.0] and idx._dist_pairs(1, [2])[0] != 1.0


def test_a_node_of_another_shape_is_at_distance_1():
    """[4,5] against [2,2,5]: the same 20 dimensions, tt_dot_product is Err(IncompatibleShapes): `else return 1.0`"""
    rng = np.random.default_rng(5)
    node = to.random_tt(rng, [4, 5], [1, 3, 1])
    same = to.random_tt(rng, [2, 2, 5], [1, 2, 2, 1])
    idx = tn.build([("tt", node), ("tt", same)], cfg(ho.EUCLIDEAN))
    q = to.random_tt(rng, [2, 2, 5], [1, 2, 3, 1])
    d = idx.cosine_distance_tt_with_norm([0, 1], q, to.tt_reconstruct(q), to.tt_norm(q))
    assert d[0] == 1.0 and d[1] != 1.0
    assert bits(d[1]) == bits(F(1.0) - so.tt_dot_product(same, q) / (to.tt_norm(same) * to.tt_norm(q)))
    # a dense query does not care about the shape: both are rows of 20
    assert (idx._dist_query([0, 1], to.tt_reconstruct(q), F(0)) != 1.0).all()


def test_the_dot_is_taken_node_first():
    """§23's fixture, query 0 and target 0: tt_dot_product(target, query) = 0xC10651E8, the swapped pair 0xC10651E6; the distance
    of the node `target` to the query differs in its last bit accordingly"""
    qs, ts = so.golden_sets()
    node, q = ts[0], qs[0]
    assert bits(so.tt_dot_product(node, q)) == 0xC10651E8 and bits(so.tt_dot_product(q, node)) == 0xC10651E6
    assert bits(to.tt_norm(node)) == 0x40B49365 and bits(to.tt_norm(q)) == 0x40DA2A7B
    idx = tn.build([("tt", node)], cfg(ho.COSINE))
    d = idx.tt_node_distance(0, q, to.tt_norm(q))
    assert bits(d) == 0x3F9BEE4C
    assert bits(F(1.0) - fbits(0xC10651E6) / (fbits(0x40B49365) * fbits(0x40DA2A7B))) == 0x3F9BEE4B


def test_the_zero_train():
    zero = to.TTVector([2, 2, 5], [1, 2, 2, 1], [np.zeros(4), np.zeros(8), np.zeros(10)])
    idx = tn.build([("tt", zero), ("tt", single(F(3.0))), ("dense", unit(20))], cfg(ho.COSINE))
    assert bits(idx.tt[0][1]) == 0 and not idx.rows[0].any()
    assert idx._dist_query([0], unit(20), F(1.0))[0] == 1.0               # mag_self == 0.0
    q = single(F(1.0))
    assert idx.tt_node_distance(0, q, to.tt_norm(q)) == 1.0
    assert idx.tt_node_distance(1, zero, to.tt_norm(zero)) == 1.0         # as a query: query_norm < 1e-10
    assert idx._dist_pairs(0, [1, 2]).tolist() == [1.0, 1.0]
    assert [s for _, s in idx.search_tt_with_ef(zero, 3, 10)] == [0.0] * 3


# ---- rules 3 and 4: one cell per pruning arm, exact integers -----------------------------------------------------------------------
def two_core_train():
    """reconstruction [19, 22, 43, 50], |v|^2 = 5194 (tests/test_hnsw_tt_oracle_cpu.py derives both by hand)"""
    g1 = np.array([[[1, 2], [3, 4]]], dtype=F)
    g2 = np.array([[[5], [6]], [[7], [8]]], dtype=F)
    return to.TTVector([2, 2], [1, 2, 1], [g1, g2])


def rank_one_train():
    """[1,2] x [3,4]: reconstruction [3, 4, 6, 8]; Gram 1 + 4 = 5, then 5 * 9 + 5 * 16 = 125 = |v|^2"""
    return to.TTVector([2, 2], [1, 1, 1], [np.array([1, 2], dtype=F), np.array([3, 4], dtype=F)])


@pytest.mark.parametrize("metric", METRICS)
def test_one_cell_per_pruning_arm(metric):
    """a = [19,22,43,50] (T), b = [3,4,6,8] (T), D = [1,0,2,0], S = Sparse([0,2,0,1]).  a.b = 803, |a-b|^2 = 3713; a.D = 105,
    |a-D|^2 = 4989; a.S = 94, |a-S|^2 = 5011.  Four elements: simd::* is the scalar tail alone, every integer sum is exact."""
    a, b = two_core_train(), rank_one_train()
    S = mo.SparseVector.from_dense(np.array([0, 2, 0, 1], dtype=F))
    idx = tn.build([("tt", a), ("tt", b), ("dense", np.array([1, 0, 2, 0], dtype=F)), ("sparse", S)], cfg(metric))
    assert idx.rows[0].tolist() == [19, 22, 43, 50] and idx.rows[1].tolist() == [3, 4, 6, 8]
    na, nb = np.sqrt(F(5194)), np.sqrt(F(125))
    assert bits(idx.tt[0][1]) == bits(na) and bits(idx.tt[1][1]) == bits(nb)
    tt_, td, ts = idx._dist_pairs(0, [1, 2, 3]).tolist()
    if metric == ho.EUCLIDEAN:
        want = [np.sqrt(F(3713)), np.sqrt(F(4989)), np.sqrt(F(5011))]
    elif metric == ho.DOT_PRODUCT:
        want = [F(-803), F(-105), F(-94)]
    else:
        want = [F(1.0) - F(803) / (na * nb),                              # 2460-2468: the cached norms
                F(1.0) - F(105) / (np.sqrt(F(5194)) * np.sqrt(F(5))),     # 2469-2480: simd::magnitude of both rows
                F(1.0 - 94.0 / (np.sqrt(np.float64(5)) * np.sqrt(np.float64(5194))))]   # 2481-2485: cosine_distance_dense, f64
    assert [bits(F(x)).item() for x in (tt_, td, ts)] == [bits(x).item() for x in want]
    # the pair in the other order is the same arm
    assert bits(idx._dist_pairs(1, [0])[0]) == bits(want[0]) and bits(idx._dist_pairs(2, [0])[0]) == bits(want[1])
    assert bits(idx._dist_pairs(3, [0])[0]) == bits(want[2])


def test_t_x_d_reads_simd_magnitude_where_the_query_side_reads_the_cached_norm():
    """the 16-element train of rule 1 beside the Dense node D = e0: the query side (the insert-time walk of D meeting T) gives
    1 - 4096 / (4096.0 * 1), the pruning arm 1 - 4096 / (0x45800003 * 1)"""
    v = np.ones(16, dtype=F)
    v[0] = 4096.0
    idx = tn.build([("tt", to.TTVector([16], [1, 1], [v])), ("dense", unit(16))], cfg(ho.COSINE))
    assert bits(idx._dist_query([0], unit(16), F(1.0))[0]) == bits(F(0.0))
    want = F(1.0) - F(4096.0) / (fbits(0x45800003) * F(1.0))
    assert want != 0.0 and bits(idx._dist_pairs(0, [1])[0]) == bits(want) and bits(idx._dist_pairs(1, [0])[0]) == bits(want)


def test_memory_stats_counts_four_bytes_per_core_float():
    a, b = two_core_train(), rank_one_train()
    S = mo.SparseVector.from_dense(np.array([0, 2, 0, 1], dtype=F))
    idx = tn.build([("tt", a), ("dense", np.zeros(4)), ("tt", b), ("sparse", S)], cfg(ho.COSINE))
    assert idx.memory_stats() == {"total_nodes": 4, "dense_count": 1, "sparse_count": 1, "tt_count": 2,
                                  "embedding_bytes": 16 + (56 + 8 * 2) + 4 * 8 + 4 * 4}


def test_new_symbols_are_exported_declared_and_bound():
    from neumann_amd import GpuHnsw, _capi
    lib = _capi.load()
    header = open(os.path.join(ROOT, "include", "neumann_gpu.h")).read()
    ffi = open(os.path.join(ROOT, "integration", "rust", "ffi.rs")).read()
    wrapper = open(os.path.join(ROOT, "integration", "rust", "gpu_index.rs")).read()
    for name in ("nmn_hnsw_insert_embedding_tt", "nmn_hnsw_tt_row", "nmn_hnsw_tt_walk_limits"):
        assert hasattr(lib, name), name
        assert re.search(rf"\b{name}\s*\(", header), name
        assert name in _capi.SIGNATURES, name
        assert re.search(rf"pub fn {name}\(", ffi), name
    assert "pub fn insert_embedding_tt(" in wrapper and "ffi::nmn_hnsw_insert_embedding_tt(" in wrapper
    for m in ("insert_embedding_tt", "tt_row", "tt_walk_limits"):
        assert callable(getattr(GpuHnsw, m))


def test_golden_fixture_is_the_twin_and_tells_the_node_kinds_apart():
    z = np.load(GOLDEN)
    trains, tt_mask, dense_q, tt_q = tn.golden_sets()
    shape, ranks, off, cores = to.pack(trains)
    assert shape.tolist() == [2, 2, 5] and np.array_equal(z["ranks"], ranks) and np.array_equal(z["core_off"], off)
    assert np.array_equal(bits(z["cores"]), bits(cores)) and np.array_equal(z["tt_mask"], tt_mask)
    assert np.array_equal(bits(z["q_cores"]), bits(to.pack(tt_q)[3])) and np.array_equal(bits(z["dense_queries"]), bits(dense_q))
    assert np.array_equal(bits(z["norms"]), bits(np.asarray([to.tt_norm(t) for t in trains], dtype=F)))
    # what the fixture script counted, pinned: the norms around 1e-10, and per metric what differs from Dense(reconstruction) nodes
    assert (int(z["norms_below"]), int(z["norms_near"])) == (23, 27)
    pinned = {"cosine": (164, 58, 60, 27), "euclidean": (0, 0, 60, 46), "dot": (0, 0, 59, 0)}
    for name, want in pinned.items():
        got = tuple(int(z[f"{name}_{c}"]) for c in ("lists_differ", "dense_differ", "tt_differ", "tt_ids_differ"))
        assert got == want, (name, got)
        assert got[2] >= 32
    assert pinned["cosine"][0] >= 1 and pinned["cosine"][1] >= 32
    # the oracle reproduces the Cosine half of the fixture
    idx = tn.golden_index(trains, tt_mask, ho.COSINE)
    assert idx.levels == z["cosine_levels"].tolist() and idx.entry_point == int(z["cosine_entry_point"])
    l0, l0cnt, up_head, up_ids = ho.golden_lists(idx)
    assert np.array_equal(l0, z["cosine_l0"]) and np.array_equal(l0cnt, z["cosine_l0cnt"])
    assert np.array_equal(up_head, z["cosine_up_head"]) and np.array_equal(up_ids, z["cosine_up_ids"])
    ids, sc, cnt = mo.answers_dense(idx, dense_q[:16], 10, 50)
    assert np.array_equal(ids, z["cosine_ids"][:16]) and np.array_equal(bits(sc), bits(z["cosine_scores"][:16]))
    ids, sc, cnt = tn.answers_tt(idx, tt_q[:16], 10, 50)
    assert np.array_equal(ids, z["cosine_tt_ids"][:16]) and np.array_equal(bits(sc), bits(z["cosine_tt_scores"][:16]))
    assert np.array_equal(cnt, z["cosine_tt_counts"][:16])
