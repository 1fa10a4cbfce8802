"""tests/_hnsw_cache_oracle.py (the cached path of lib.rs:1976-2001 / 1622-1646) against hand-made cases."""
import numpy as np

from tests import _hnsw_cache_oracle as co
from tests import _hnsw_oracle as ho

F = np.float32
ROWS = np.eye(6, dtype=F)[:, :4].copy()      # rows 0-3: the unit vectors of 4 dimensions; rows 4, 5: zero rows
ROWS[4] = [0.9, 0.1, 0.0, 0.0]
ROWS[5] = [1.0, 0.0, 0.0, 0.0]               # an exact duplicate of row 0: equal scores, order decided by the walk
Q = np.array([1.0, 0.0, 0.0, 0.0], F)


def index():
    return ho.build(ROWS)


def test_plain_keys_sorted_descending_and_truncated():
    o = index()
    keys = [f"k{i}" for i in range(6)]
    walk = o.search(Q, 6)
    got = co.cached_search(o, keys, co.embedding_prefix(), Q, 6)
    assert [k for k, _ in got] == [f"k{n}" for n, _ in walk]          # the walk is already descending: the stable sort keeps it
    assert [s.tobytes() for _, s in got] == [F(s).tobytes() for _, s in walk]
    assert {got[0][0], got[1][0]} == {"k0", "k5"} and got[0][1] == got[1][1] == F(1.0) and got[2][0] == "k4"
    assert all(a[1] >= b[1] for a, b in zip(got, got[1:]))
    assert co.cached_search(o, keys, co.embedding_prefix(), Q, 2) == got[:2]


def test_mapping_shorter_than_the_index_drops_ids():
    o = index()
    got = co.cached_search(o, ["k0", "k1", "k2"], co.embedding_prefix(), Q, 6)
    assert sorted(k for k, _ in got) == ["k0", "k1", "k2"] and got[0][0] == "k0"
    got = co.cached_search(o, ["k0"], co.embedding_prefix(), ROWS[1], 1)    # top_k is spent on the walk, before ids are dropped
    assert got == []


def test_storage_keys_are_stripped_plain_keys_are_kept():
    o = index()
    prefix = co.collection_embedding_prefix("docs")
    assert prefix == "coll:docs:emb:"
    mapping = [prefix + "d0", "d1", "emb:d2", "coll:other:emb:d3", prefix + "d4", prefix]
    got = dict(co.cached_search(o, mapping, prefix, Q, 6))
    assert set(got) == {"d0", "d1", "emb:d2", "coll:other:emb:d3", "d4", ""}
    got = dict(co.cached_search(o, mapping, co.embedding_prefix(), Q, 6))
    assert set(got) == {prefix + "d0", "d1", "d2", "coll:other:emb:d3", prefix + "d4", prefix}


def test_a_user_key_that_starts_with_the_prefix_loses_it_once():
    o = index()
    mapping = ["emb:x", "emb:emb:y", "z", "k3", "k4", "k5"]
    got = [k for k, _ in co.cached_search(o, mapping, co.embedding_prefix(), ROWS[1], 6)]
    assert "emb:y" in got and "x" in got and "z" in got and "emb:x" not in got


def test_empty_mapping_and_no_entry_fall_through():
    o = index()
    assert co.cached_search(o, [], co.embedding_prefix(), Q, 3) is None
    assert co.cached_search(o, None, co.embedding_prefix(), Q, 3) is None


def test_empty_index_under_a_mapping_answers_nothing():
    assert co.cached_search(None, ["a", "b"], co.embedding_prefix(), Q, 3) == []
    assert co.cached_search(ho.HNSWIndex(), ["a", "b"], co.embedding_prefix(), Q, 3) == []


def test_stable_sort_keeps_the_walk_order_of_equal_scores():
    class Fixed:  # a walk that returns equal scores out of order
        def search(self, q, k):
            return [(2, F(0.5)), (0, F(0.75)), (1, F(0.5)), (3, F(0.75))][:k]
    got = co.cached_search(Fixed(), ["a", "b", "c", "d"], "emb:", Q, 4)
    assert got == [("a", F(0.75)), ("d", F(0.75)), ("c", F(0.5)), ("b", F(0.5))]
    assert co.cached_search(Fixed(), ["a", "b", "c", "d"], "emb:", Q, 3) == [("a", F(0.75)), ("c", F(0.5)), ("b", F(0.5))]
