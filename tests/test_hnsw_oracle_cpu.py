"""tests/_hnsw_oracle.py against what the reference itself pins (its own unit tests, restated), against hand-derived heap
layouts and level values, against structural invariants of a built graph, and against tests/golden/hnsw_small.npz."""
import math
import os

import numpy as np
import pytest

from oracle import oracle_c as oc
from tests import _hnsw_oracle as ho

F = np.float32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hnsw_small.npz")


# ---- the reference's own assertions -------------------------------------------------------------------------------------------
def test_hnsw_basic_insert_and_search():  # hnsw.rs:2817-2830
    idx = ho.HNSWIndex()
    for v in ([1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]):
        idx.insert(v)
    assert len(idx) == 3
    res = idx.search([1.0, 0.0, 0.0], 3)
    assert len(res) == 3
    assert res[0][0] == 0
    assert abs(float(res[0][1]) - 1.0) < 1e-6


def test_hnsw_empty_search():  # hnsw.rs:2833-2837
    assert ho.HNSWIndex().search([1.0, 0.0], 5) == []


def test_hnsw_search_euclidean_basic():  # hnsw.rs:4990-5002
    idx = ho.HNSWIndex(ho.HNSWConfig().with_distance_metric(ho.EUCLIDEAN))
    for v in ([0.0, 0.0], [1.0, 0.0], [10.0, 0.0]):
        idx.insert(v)
    res = idx.search([0.5, 0.0], 2)
    assert len(res) == 2
    assert any(i in (0, 1) for i, _ in res)
    # both are at distance 0.5: similarity 1 / (1 + 0.5)
    assert sorted(i for i, _ in res) == [0, 1] and all(s == F(1.0) / F(1.5) for _, s in res)


def test_hnsw_search_dot_product_basic():  # hnsw.rs:5005-5017
    idx = ho.HNSWIndex(ho.HNSWConfig().with_distance_metric(ho.DOT_PRODUCT))
    for v in ([1.0, 0.0], [2.0, 0.0], [0.5, 0.0]):
        idx.insert(v)
    res = idx.search([1.0, 0.0], 3)
    assert len(res) == 3
    assert res[0][0] == 1 and res[0][1] == F(2.0)


def create_test_vector(dim, seed):  # vector_engine/src/lib.rs:4029-4038
    out = []
    for i in range(dim):
        x = F(seed * 31 + i * 17)
        out.append(F(math.sin(float(x * F(0.0001)))) * (F(seed + i) * F(0.001)))
    return np.asarray(out, dtype=F)


def test_engine_search_with_hnsw():  # lib.rs:4643-4667
    keys = sorted(f"vec{i}" for i in range(100))  # list_keys() order is the store's; any fixed order serves the assertion
    rows = np.stack([create_test_vector(32, int(k[3:])) for k in keys])
    idx = ho.build(rows)
    res = ho.search_with_hnsw(idx, keys, create_test_vector(32, 42), 5)
    assert len(res) == 5
    assert any("42" in key for key, _ in res)


def test_engine_hnsw_empty_query_error():  # lib.rs:4670-4677
    with pytest.raises(ValueError, match="Empty vector provided"):
        ho.search_with_hnsw(ho.HNSWIndex(), [], [], 5)


def test_engine_hnsw_zero_top_k_error():  # lib.rs:4680-4687
    with pytest.raises(ValueError, match="Invalid top_k"):
        ho.search_with_hnsw(ho.HNSWIndex(), [], [1.0], 0)


def test_capacity_error_text():  # hnsw.rs:102-107, 1947-1955
    idx = ho.HNSWIndex(ho.HNSWConfig(max_nodes=2))
    idx.insert([1.0, 0.0])
    idx.insert([0.0, 1.0])
    with pytest.raises(ho.CapacityExceeded, match=r"HNSW index at capacity: 2 nodes \(limit: 2\)"):
        idx.insert([1.0, 1.0])
    assert len(idx) == 2


def test_estimate_hnsw_memory_formula():  # lib.rs:2489-2509
    assert ho.estimate_hnsw_memory(0, 128) == 0
    assert ho.estimate_hnsw_memory(1000, 128) == 1000 * 128 * 4 + 1000 * 16 * 2 * 8 + 1000 * 32


# ---- the level generator --------------------------------------------------------------------------------------------------------
def test_level_generator_first_values():
    """hnsw.rs:1631-1651.  By hand for the first draw: seed 42; 42 << 13 = 344064, 42 ^ 344064 = 344106; 344106 >> 7 = 2688,
    344106 ^ 2688 = 346794; 346794 << 17 = 45454983168, 346794 ^ 45454983168 = 45454805674.  f = 45454805674 / 2^64 =
    2.46411e-9, -ln f = 19.82144; times 1 / ln 16 = 0.360674 -> 7.149 -> 7; times 1 / ln 8 = 0.480898 -> 9.53 -> 9; times
    1 / ln 32 = 0.288539 -> 5.72 -> 5.  The rest of each list comes from the same arithmetic in plain Python integers and f64."""
    assert 42 ^ (42 << 13) == 344106 and 344106 ^ (344106 >> 7) == 346794 and 346794 ^ (346794 << 17) == 45454805674
    want = {16: [7, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0],
            8: [9, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 0, 0, 0],
            32: [5, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0]}
    for m, levels in want.items():
        idx = ho.HNSWIndex(ho.HNSWConfig(m=m))
        assert [idx.random_level() for _ in range(24)] == levels
        s, plain = 42, []
        for _ in range(24):
            s ^= (s << 13) % 2**64
            s ^= s >> 7
            s ^= (s << 17) % 2**64
            plain.append(min(math.floor(-math.log(s / 2.0**64) / math.log(m)), 32))
        # (dividing by ln m instead of multiplying by 1 / ln m: the same integers unless a product sits on an integer boundary)
        assert plain == levels
    # over many draws levels above 0 do occur and follow the geometric law roughly
    idx = ho.HNSWIndex()
    lv = np.asarray([idx.random_level() for _ in range(20000)])
    assert 0.04 < np.mean(lv >= 1) < 0.09 and lv.max() <= 32


# ---- BinaryHeap: layouts derived by hand ----------------------------------------------------------------------------------------
def _ids(seq):
    return [e[1] for e in seq]


def test_heap_equal_keys_max():
    """MaxNeighbor, all keys equal.  Pushes never move anything (an element equal to its parent stops at once): the vector is the
    push order.  Three elements a b c: pop takes c into the root of [a b], the hole walks to the bottom (only child b moves up), c
    lands below it: [b c], a popped; then b, then c.  Four elements a b c d: pop puts d at the root of [a b c]; children b, c are
    equal so the RIGHT one (c) moves up, d lands in its place: [c b d], a popped; next pop: d to the root of [c b], only child b moves
    up: [b d], c popped; then b, then d."""
    h = ho.BinaryHeap(ho.max_neighbor_le)
    for name in "abc":
        h.push((1.0, name))
    assert _ids(h.into_vec()) == list("abc")
    assert h.pop()[1] == "a" and _ids(h.into_vec()) == ["b", "c"]
    assert [h.pop()[1], h.pop()[1]] == ["b", "c"] and h.pop() is None
    for name in "abcd":
        h.push((1.0, name))
    assert h.pop()[1] == "a" and _ids(h.into_vec()) == ["c", "b", "d"]
    assert h.pop()[1] == "c" and _ids(h.into_vec()) == ["b", "d"]
    assert [h.pop()[1], h.pop()[1]] == ["b", "d"]


def test_heap_mixed_keys_max():
    """MaxNeighbor, pushes a2 b1 c2 d3 e2.  a: [a]; b1 <= a2 stays: [a b]; c2 <= a2 stays: [a b c]; d3 > b1 and > a2 rises to the
    root: [d a c b]; e2 <= a2 (its parent, slot 1) stays: [d a c b e].  pop 1: e to the root of [d a c b] -> hole follows the right child on
    the tie a2 == c2: c up, e lands at slot 2: [c a e b], d popped.  pop 2: b to the root of [c a e]: tie a2 == e2 -> e up, b
    lands: [e a b], c popped.  pop 3: b to the root of [e a]: a up: [a b], e popped.  Then a, b."""
    h = ho.BinaryHeap(ho.max_neighbor_le)
    for d, name in ((2.0, "a"), (1.0, "b"), (2.0, "c"), (3.0, "d"), (2.0, "e")):
        h.push((d, name))
    assert _ids(h.into_vec()) == list("dacbe")
    assert h.peek()[1] == "d"
    assert h.pop()[1] == "d" and _ids(h.into_vec()) == list("caeb")
    assert h.pop()[1] == "c" and _ids(h.into_vec()) == list("eab")
    assert h.pop()[1] == "e" and _ids(h.into_vec()) == list("ab")
    assert [h.pop()[1], h.pop()[1]] == ["a", "b"]


def test_heap_mixed_keys_min():
    """Neighbor (reversed order: the smallest distance is the greatest element), the same pushes.  a: [a]; b1 beats a2: [b a];
    c2 does not beat b1: [b a c]; d3 does not beat a2: [b a c d]; e2 does not beat a2 (equal): [b a c d e].  pop 1: e to the root of
    [b a c d]: children a2, c2 tie -> the right one, c, moves up; slot 2 has no children; e lands there: [c a e d], b popped.
    pop 2: d to the root of [c a e]: tie a2 == e2 -> e up, d lands: [e a d], c popped.  pop 3: d to the root of [e a]: a up:
    [a d], e popped.  Then a, d.  So among the three entries at distance 2 the pop order is c, e, a — neither id nor push order."""
    h = ho.BinaryHeap(ho.neighbor_le)
    for d, name in ((2.0, "a"), (1.0, "b"), (2.0, "c"), (3.0, "d"), (2.0, "e")):
        h.push((d, name))
    assert _ids(h.into_vec()) == list("bacde")
    assert h.pop()[1] == "b" and _ids(h.into_vec()) == list("caed")
    assert h.pop()[1] == "c" and _ids(h.into_vec()) == list("ead")
    assert h.pop()[1] == "e" and _ids(h.into_vec()) == list("ad")
    assert [h.pop()[1], h.pop()[1]] == ["a", "d"]


def test_heap_orders_distinct_keys():
    rng = np.random.default_rng(3)
    keys = rng.permutation(500).astype(float)
    for le, rev in ((ho.max_neighbor_le, True), (ho.neighbor_le, False)):
        h = ho.BinaryHeap(le)
        for i, d in enumerate(keys):
            h.push((d, i))
        assert [h.pop()[0] for _ in range(500)] == sorted(keys, reverse=rev)


# ---- arithmetic -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [1, 3, 7, 8, 9, 20, 64, 100])
def test_distances_against_the_c_oracle_and_scalar_chains(dim):
    rng = np.random.default_rng(dim)
    A = rng.standard_normal((6, dim)).astype(F)
    q = rng.standard_normal(dim).astype(F)
    dots = ho.dot_product_rows(A, q)
    eu = ho.euclidean_distance_rows(A, q)
    for i in range(6):
        assert dots[i] == oc.dot8(A[i], q)
        # the 8-lane Euclidean as explicit scalar chains (hnsw.rs:234-261)
        acc = [F(0)] * 8
        for c in range(dim // 8):
            for lane in range(8):
                d = A[i, 8 * c + lane] - q[8 * c + lane]
                acc[lane] = acc[lane] + d * d
        r = F(-0.0)
        for lane in range(8):
            r = r + acc[lane]
        for j in range(dim // 8 * 8, dim):
            d = A[i, j] - q[j]
            r = r + d * d
        assert eu[i] == np.sqrt(r)
    assert ho.magnitude(q) == oc.magnitude(q)


def test_zero_magnitude_rule():  # hnsw.rs:1040-1042, 2447-2448
    idx = ho.HNSWIndex()
    idx.insert(np.zeros(4, F))
    idx.insert(np.asarray([1, 0, 0, 0], F))
    assert idx._dist_query([0, 1], np.asarray([1, 0, 0, 0], F), F(1.0)).tolist() == [1.0, 0.0]
    assert idx._dist_query([0, 1], np.zeros(4, F), F(0.0)).tolist() == [1.0, 1.0]
    assert idx._dist_pairs(0, [1]).tolist() == [1.0] and idx._dist_pairs(1, [0]).tolist() == [1.0]


# ---- structure of a built graph ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", [ho.COSINE, ho.EUCLIDEAN, ho.DOT_PRODUCT])
def test_graph_invariants(metric):
    rng = np.random.default_rng(11 + metric)
    rows = rng.standard_normal((400, 12)).astype(F)
    rows[::5] = rows[3]  # duplicates
    idx = ho.build(rows, ho.HNSWConfig.high_speed().with_distance_metric(metric))
    cfg = idx.config
    assert len(idx) == 400 and idx.levels[idx.entry_point] == idx.max_layer == max(idx.levels)
    for node in range(400):
        assert len(idx.neighbors[node]) == idx.levels[node] + 1
        for layer, lst in enumerate(idx.neighbors[node]):
            assert lst == sorted(set(lst)) and node not in lst
            assert len(lst) <= (cfg.m0 if layer == 0 else cfg.m)
            assert all(idx.levels[t] >= layer for t in lst)


# ---- the golden file ----------------------------------------------------------------------------------------------------------------
def test_golden_file_is_what_the_oracle_builds():
    g = np.load(GOLDEN)
    rows, queries = ho.golden_corpus()
    assert np.array_equal(g["rows"], rows) and np.array_equal(g["queries"], queries)
    assert g["config"].tolist() == [16, 32, 200, 50, ho.COSINE]
    idx = ho.build(rows)
    assert g["levels"].tolist() == idx.levels and int(g["entry_point"]) == idx.entry_point and int(g["max_layer"]) == idx.max_layer
    l0, l0cnt, up_head, up_ids = ho.golden_lists(idx)
    assert np.array_equal(g["l0"], l0) and np.array_equal(g["l0cnt"], l0cnt)
    assert np.array_equal(g["up_head"], up_head) and np.array_equal(g["up_ids"], up_ids)
    ids, sc, cnt = ho.padded_answers(idx, queries, int(g["k"]))
    assert np.array_equal(g["ids"], ids) and np.array_equal(g["scores"].view(np.uint32), sc.view(np.uint32))
    assert np.array_equal(g["counts"], cnt)
    ids, sc, cnt = ho.padded_answers(idx, queries, int(g["k"]), ef=int(g["ef2"]))
    assert np.array_equal(g["ids_ef2"], ids) and np.array_equal(g["scores_ef2"].view(np.uint32), sc.view(np.uint32))
    # its own consistency: duplicated rows really tie in the answers, and the first eight queries find a copy of themselves
    for i in range(8):
        assert np.array_equal(rows[int(g["ids"][i, 0])], queries[i])
    assert os.path.getsize(GOLDEN) < 1 << 20
