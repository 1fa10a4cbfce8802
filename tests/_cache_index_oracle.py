"""CPU restatement of the reference's semantic-cache index, `tensor_cache::CacheIndex` — TEST INFRASTRUCTURE ONLY.

Written from the reference's text, independently of the product; paths relative to the reference root:
  tensor_cache/src/index.rs   CacheIndex 30-45, insert 91-118, insert_sparse 123-148, insert_auto 153-166, search 172-179,
                              search_with_metric 186-272, search_sparse 278-285, search_sparse_with_metric 291-375, remove 383-391,
                              contains / len / is_empty / dimension 395-414, clear 420-428, keys 432-434, memory_stats 440-442,
                              get_embedding 446-450
  tensor_store/src/sparse_vector.rs   sparsity 302-308

It sits on `_hnsw_mixed_oracle.HNSWMixedIndex` (the walk, Dense and Sparse nodes), `_hnsw_sparse_query_oracle.SparseQuery` and the
metric functions of `_xmetric_oracle`, which work on anything with `positions` / `values` in stored order: a Sparse node or a sparse
query goes into `compute` as its stored entries ARE (229-232, 332-334), duplicated positions included, a Dense node as
`SparseVector::from_dense(row)` (224-228).
"""
import numpy as np

from tests import _hnsw_mixed_oracle as mo
from tests import _hnsw_oracle as ho
from tests import _xmetric_oracle as xo

F = np.float32
U64_MAX = (1 << 64) - 1


class Entries:
    """the stored entries of a SparseVector as `_xmetric_oracle` reads them: positions, and the f32 values as Python floats (f64)"""

    def __init__(self, sv):
        self.dimension = sv.dimension
        self.positions = [int(p) for p in sv.positions]
        self.values = [float(v) for v in np.asarray(sv.values, dtype=F).tolist()]


def candidate_count(k):
    """`(k * 3).max(10)` (index.rs:206, 311) in 64 bits"""
    return max(min(3 * int(k), U64_MAX), 10)


def similarity(metric, query_entries, stored_entries):
    """metric.to_similarity(metric.compute(query, stored)) (226-227)"""
    return F(xo.to_similarity(metric, xo.compute(metric, query_entries, stored_entries)))


def stored_entries(idx, node):
    """what index.get_embedding(node) goes into compute as (223-232)"""
    sv = idx.sparse.get(node)
    return Entries(sv) if sv is not None else xo.Sparse(idx.rows[node])


def rescore(idx, live, candidates, query_entries, k, threshold, metric):
    """212-269 on the walk's candidate nodes: -> [(node, similarity f32)].  `live(node)`: node_to_key has the node."""
    thr = F(threshold)
    results = []
    for node in candidates:
        if not live(node):
            continue
        sim = similarity(metric, query_entries, stored_entries(idx, node))
        if sim >= thr:   # f32 >= f32: false when either is NaN, true on equality
            results.append((node, sim))
    # sort_by(|a, b| b.similarity.partial_cmp(&a.similarity).unwrap_or(Equal)): stable, descending (no NaN passed the threshold)
    results.sort(key=lambda t: -float(t[1]))
    return results[:k]


def rescore_densified(idx, live, candidates, query_entries, k, threshold, metric):
    """what a re-rank of the to_dense() ROWS would answer (every node as from_dense(row)): NOT the reference — the twin a test
    holds answers against, to show that they depend on the stored entries"""
    thr = F(threshold)
    results = []
    for node in candidates:
        if live(node):
            sim = similarity(metric, query_entries, xo.Sparse(idx.rows[node]))
            if sim >= thr:
                results.append((node, sim))
    results.sort(key=lambda t: -float(t[1]))
    return results[:k]


def search_nodes(idx, live, query, k, threshold, metric):
    """search_with_metric (186-272) with nodes in place of keys.  The walk is idx.search(query, c): the INDEX's metric."""
    if len(idx) == 0:
        return []
    q = np.asarray(query, dtype=F)
    cands = [nid for nid, _ in idx.search(q, candidate_count(k))]
    return rescore(idx, live, cands, xo.Sparse(q), k, threshold, metric)


def search_nodes_sparse(idx, live, sq, k, threshold, metric):
    """search_sparse_with_metric (291-375) with nodes in place of keys; sq: a SparseQuery / SparseVector"""
    if len(idx) == 0:
        return []
    cands = [nid for nid, _ in idx.search_sparse_with_ef(sq, candidate_count(k), idx.config.ef_search)]
    return rescore(idx, live, cands, Entries(sq), k, threshold, metric)


class DimensionMismatch(Exception):
    def __init__(self, expected, got):
        super().__init__(f"dimension mismatch: expected {expected}, got {got}")
        self.expected, self.got = expected, got


class CacheIndex:
    def __init__(self, dimension, config=None, metric=None):
        self.dimension = int(dimension)
        self.config = config or ho.HNSWConfig()
        self.distance_metric = metric or xo.Metric(xo.COSINE)
        self.index = mo.HNSWMixedIndex(self.config)
        self.key_to_node = {}
        self.node_to_key = {}
        self.entry_count = 0

    def metric(self):
        return self.distance_metric

    def _bind(self, key, insert):
        is_new = key not in self.key_to_node
        if not is_new:
            del self.key_to_node[key]   # (104: node_to_key keeps the old node)
        node = insert()
        self.key_to_node[key] = node
        self.node_to_key[node] = key
        if is_new:
            self.entry_count += 1
        return node

    def insert(self, key, embedding):
        v = np.asarray(embedding, dtype=F).reshape(-1)
        if v.size != self.dimension:
            raise DimensionMismatch(self.dimension, v.size)
        return self._bind(key, lambda: self.index.insert(v))

    def insert_sparse(self, key, sv):
        if sv.dimension != self.dimension:
            raise DimensionMismatch(self.dimension, sv.dimension)
        return self._bind(key, lambda: self.index.insert_sparse(sv))

    def insert_auto(self, key, embedding, sparsity_threshold):
        v = np.asarray(embedding, dtype=F).reshape(-1)
        sv = mo.SparseVector.from_dense(v)
        sparsity = F(0.0) if sv.dimension == 0 else F(1.0) - (F(len(sv)) / F(sv.dimension))
        if sparsity >= F(sparsity_threshold):
            return self.insert_sparse(key, sv)
        return self.insert(key, v)

    def _keys(self, results):
        return [(self.node_to_key[node], sim) for node, sim in results]

    def search_with_metric(self, query, k, threshold, metric):
        q = np.asarray(query, dtype=F).reshape(-1)
        if q.size != self.dimension:
            raise DimensionMismatch(self.dimension, q.size)
        return self._keys(search_nodes(self.index, self.node_to_key.__contains__, q, k, threshold, metric))

    def search(self, query, k, threshold):
        return self.search_with_metric(query, k, threshold, self.distance_metric)

    def search_sparse_with_metric(self, sq, k, threshold, metric):
        if sq.dimension != self.dimension:
            raise DimensionMismatch(self.dimension, sq.dimension)
        return self._keys(search_nodes_sparse(self.index, self.node_to_key.__contains__, sq, k, threshold, metric))

    def search_sparse(self, sq, k, threshold):
        return self.search_sparse_with_metric(sq, k, threshold, self.distance_metric)

    def remove(self, key):
        node = self.key_to_node.pop(key, None)
        if node is None:
            return False
        self.node_to_key.pop(node, None)
        self.entry_count -= 1
        return True

    def contains(self, key):
        return key in self.key_to_node

    def __len__(self):
        return self.entry_count

    def is_empty(self):
        return self.entry_count == 0

    def clear(self):
        self.index = mo.HNSWMixedIndex(self.config)   # ids from 0 again, the level generator at its seed again
        self.key_to_node.clear()
        self.node_to_key.clear()
        self.entry_count = 0

    def keys(self):
        return list(self.key_to_node)

    def memory_stats(self):
        return self.index.memory_stats()

    def get_embedding(self, key):
        """-> ("dense", row) / ("sparse", SparseVector) / None"""
        node = self.key_to_node.get(key)
        if node is None:
            return None
        sv = self.index.sparse.get(node)
        return ("sparse", sv) if sv is not None else ("dense", self.index.rows[node].copy())


def padded(results, k):
    """the library's layout: ids u64 [nq][max(k, 1)] (unused UINT64_MAX), similarities f32 (unused -inf), counts u32"""
    return mo.padded(results, max(k, 1))
