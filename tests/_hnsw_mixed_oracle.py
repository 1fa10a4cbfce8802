"""CPU restatement of the reference's HNSW index holding Sparse AND Dense nodes — TEST INFRASTRUCTURE ONLY.

Written from the reference's text, independently of the product (neumann_amd/csrc/nmn_hnsw.hip); paths relative to the
reference root:
  tensor_store/src/sparse_vector.rs  try_from_parts 155-193, try_from_dense 212-236, to_dense 400-406, dot / dot_f64 414-443 (a
                                     two-pointer merge, the accumulator `0.0_f64`: +0.0, no Sum), dot_dense 450-466 and
                                     magnitude / magnitude_f64 548-559 (`Iterator::sum::<f64>()`: a fold from -0.0),
                                     cosine_similarity 583-600, cosine_distance_dense 606-632, euclidean_distance 942-1006 (the
                                     f64 union merge, sqrt, clamp to f32::MAX, cast), memory_bytes 1064-1068
  tensor_store/src/hnsw.rs           EmbeddingStorage::cosine_distance_dense 1035-1045, cosine_distance_sparse 1069-1079,
                                     euclidean_distance_dense / _sparse 1084-1114, dot_product_distance_* 1136-1145, memory_bytes
                                     1225-1235, insert_sparse 1660-1662, insert_auto 1671-1680, the insert-time query
                                     `embedding.to_dense()` 1985, try_cosine / euclidean / dot_product_distance (the Sparse x Sparse
                                     and Dense x Sparse arms) 2437-2459, 2554-2565, 2637-2643

`HNSWMixedIndex` is `_hnsw_oracle.HNSWIndex` with a kind per node; the walk, the heaps and the pruning loop are that class's, only
the two distance hooks and the insertion's bookkeeping change.  Python floats ARE f64; every f64 product of two f32 is exact, every
addition rounds once, `np.float32(x)` is the one cast (round to nearest even).
"""
import math

import numpy as np

from tests import _hnsw_oracle as ho
from tests._hnsw_sparse_query_oracle import SparseQuery

F = np.float32
D = np.float64
F32_MAX = float(np.finfo(np.float32).max)
SIZE_OF_SPARSE_VECTOR = 56   # usize dimension + two Vecs of three words each, 64-bit target


class SparseVector(SparseQuery):
    """SparseQuery (from_parts, from_dense, to_dense, dot_dense, magnitude) plus what a stored Sparse node needs."""

    def _fold(self, products):
        """Iterator::sum::<f64>(): a left-to-right fold from -0.0 (np.add.accumulate adds in sequence, one rounding per add)"""
        chain = np.concatenate([np.array([-0.0]), np.asarray(products, dtype=D)])
        return float(np.add.accumulate(chain)[-1])

    def _pos(self):
        return np.asarray(self.positions, dtype=np.int64)

    def magnitude_f64(self):
        v = self.values.astype(D)
        return math.sqrt(self._fold(v * v))        # a product of two f32 is exact in f64

    def dot_dense_f64(self, dense):
        return self._fold(self.values.astype(D) * np.asarray(dense, dtype=F)[self._pos()].astype(D))

    def dot_dense(self, dense):
        return _cast(self.dot_dense_f64(dense))

    def dot_f64(self, other):
        result = 0.0
        i = j = 0
        a, b = self.positions, other.positions
        while i < len(a) and j < len(b):
            if a[i] == b[j]:
                result += float(self.values[i]) * float(other.values[j])
                i += 1
                j += 1
            elif a[i] < b[j]:
                i += 1
            else:
                j += 1
        return result

    def dot(self, other):
        return _cast(self.dot_f64(other))

    def euclidean_distance(self, other):
        s = 0.0
        i = j = 0
        a, b = self.positions, other.positions
        while i < len(a) or j < len(b):
            if i >= len(a):
                d = float(other.values[j])
                j += 1
            elif j >= len(b):
                d = float(self.values[i])
                i += 1
            elif a[i] == b[j]:
                d = float(self.values[i]) - float(other.values[j])
                i += 1
                j += 1
            elif a[i] < b[j]:
                d = float(self.values[i])
                i += 1
            else:
                d = -float(other.values[j])
                j += 1
            s += d * d
        dist = math.sqrt(s)
        return F(F32_MAX) if dist > F32_MAX else _cast(dist)

    def cosine_similarity(self, other):
        dot = self.dot_f64(other)
        ma, mb = self.magnitude_f64(), other.magnitude_f64()
        if ma == 0.0 or mb == 0.0:
            return F(0.0)
        r = _div(dot, ma * mb)
        if math.isnan(r) or math.isinf(r):
            return F(0.0)
        return _cast(min(max(r, -1.0), 1.0))

    def cosine_distance_dense(self, dense):
        dot = self.dot_dense_f64(dense)
        ms = self.magnitude_f64()
        d = np.asarray(dense, dtype=F).astype(D)
        md = math.sqrt(self._fold(d * d))
        if ms == 0.0 or md == 0.0:
            return F(1.0)
        r = _div(dot, ms * md)
        if math.isnan(r) or math.isinf(r):
            return F(1.0)
        return _cast(1.0 - min(max(r, -1.0), 1.0))

    def memory_bytes(self):
        return SIZE_OF_SPARSE_VECTOR + 8 * len(self.positions)   # capacity taken as len (a cloned Vec)

    def has_duplicates(self):
        return len(set(self.positions)) != len(self.positions)


def _cast(x):
    with np.errstate(over="ignore"):
        return F(x)


def _div(a, b):
    try:
        return a / b
    except ZeroDivisionError:
        return math.nan if a == 0.0 or math.isnan(a) else math.copysign(math.inf, a) * math.copysign(1.0, b)


def _cosine(dot, mag_self, mag_query):
    """1.0 - dot / (mag_self * mag_query) in f32, 1.0 when a magnitude == 0.0"""
    dot, mag_self, mag_query = F(dot), F(mag_self), F(mag_query)
    if mag_self == 0 or mag_query == 0:
        return F(1.0)
    with np.errstate(all="ignore"):
        return F(1.0) - (dot / (mag_self * mag_query))


class HNSWMixedIndex(ho.HNSWIndex):
    def __init__(self, config=None):
        super().__init__(config)
        self.sparse = {}      # node -> SparseVector; every other node is Dense
        self._sq = None       # the SparseVector query of a search_sparse walk

    def kind(self, node):
        return "sparse" if node in self.sparse else "dense"

    # ---- the query side -----------------------------------------------------------------------------------------------------
    def _qmag(self, q):
        if self._sq is not None:
            return self._sq.magnitude() if self.config.distance_metric == ho.COSINE else F(0)
        return super()._qmag(q)

    def _dense_nodes_query(self, ids, q, qmag):
        """Dense nodes: distance_dense, or distance_sparse through dot_dense (Cosine / DotProduct) / to_dense (Euclidean)"""
        metric = self.config.distance_metric
        if self._sq is None or metric == ho.EUCLIDEAN:
            evals = self.distance_evals
            d = ho.HNSWIndex._dist_query(self, ids, q, qmag)
            self.distance_evals = evals
            return d
        dot = self._sq.dot_dense_rows(self.rows[ids])
        if metric == ho.DOT_PRODUCT:
            return -dot
        return np.array([_cosine(x, self.mags[i], qmag) for x, i in zip(dot, ids)], dtype=F)

    def _sparse_node_query(self, node, q, qmag):
        metric = self.config.distance_metric
        s = self.sparse[node]
        if self._sq is None:   # a dense query
            if metric == ho.EUCLIDEAN:
                return ho.euclidean_distance_rows(s.to_dense()[None, :], q)[0]
            dot = s.dot_dense(q)
        else:
            if metric == ho.EUCLIDEAN:
                return s.euclidean_distance(self._sq)
            dot = s.dot(self._sq)
        if metric == ho.DOT_PRODUCT:
            return -dot
        return _cosine(dot, s.magnitude(), qmag)

    def _dist_query(self, ids, q, qmag):
        ids = list(ids)
        self.distance_evals += len(ids)
        out = np.empty(len(ids), dtype=F)
        dense = [(k, i) for k, i in enumerate(ids) if i not in self.sparse]
        if dense:
            out[[k for k, _ in dense]] = self._dense_nodes_query([i for _, i in dense], q, qmag)
        for k, i in enumerate(ids):
            if i in self.sparse:
                out[k] = self._sparse_node_query(i, q, qmag)
        return out

    # ---- the pruning side -------------------------------------------------------------------------------------------------------
    def _pair(self, a, b):
        metric = self.config.distance_metric
        sa, sb = self.sparse.get(a), self.sparse.get(b)
        if sa is not None and sb is not None:
            if metric == ho.EUCLIDEAN:
                return sa.euclidean_distance(sb)
            if metric == ho.DOT_PRODUCT:
                return -sa.dot(sb)
            return F(1.0) - sa.cosine_similarity(sb)
        s, v = (sa, self.rows[b]) if sa is not None else (sb, self.rows[a])
        if metric == ho.EUCLIDEAN:
            return ho.euclidean_distance_rows(s.to_dense()[None, :], v)[0]
        if metric == ho.DOT_PRODUCT:
            return -s.dot_dense(v)
        return s.cosine_distance_dense(v)

    def _dist_pairs(self, a_id, ids):
        ids = list(ids)
        out = np.empty(len(ids), dtype=F)
        plain = [k for k, i in enumerate(ids) if a_id not in self.sparse and i not in self.sparse]
        if plain:
            out[plain] = ho.HNSWIndex._dist_pairs(self, a_id, [ids[k] for k in plain])
        for k, i in enumerate(ids):
            if a_id in self.sparse or i in self.sparse:
                out[k] = self._pair(a_id, i)
        return out

    # ---- insertion ----------------------------------------------------------------------------------------------------------
    def _insert_embedding(self, dense_row, sv):
        """try_insert_embedding: the parent's insert with the kind and the Sparse node's magnitude() in place before the walk"""
        node_id = self.n
        if sv is not None:
            self.sparse[node_id] = sv
        try:
            got = super().insert(dense_row)   # the query is embedding.to_dense() (hnsw.rs:1985): a dense walk
        except Exception:
            self.sparse.pop(node_id, None)
            raise
        return got

    def insert(self, vector):
        return self._insert_embedding(np.asarray(vector, dtype=F), None)

    def insert_sparse(self, sv):
        return self._insert_embedding(sv.to_dense(), sv)

    def insert_auto(self, vector):
        v = np.asarray(vector, dtype=F)
        nnz = int(np.count_nonzero(v != 0))            # NaN != 0.0 is true
        sparsity = F(1.0) - (F(nnz) / F(v.size))
        if sparsity >= F(self.config.sparsity_threshold):   # false for a NaN threshold
            return self.insert_sparse(SparseVector.from_dense(v))
        return self.insert(v)

    # ---- searches -----------------------------------------------------------------------------------------------------------
    def search_sparse_with_ef(self, sq, k, ef):
        w = HNSWMixedIndex.__new__(HNSWMixedIndex)
        w.__dict__.update(self.__dict__)
        w._sq = sq
        w.distance_evals = 0
        res = w.search_with_ef(sq.to_dense(), k, ef)
        self.distance_evals += w.distance_evals
        return res

    def to_dense_rows(self):
        return self.rows[:self.n].copy()

    def memory_stats(self):
        dim = self.rows.shape[1] if self.rows is not None else 0
        ns = len(self.sparse)
        return {"total_nodes": self.n, "dense_count": self.n - ns, "sparse_count": ns,
                "embedding_bytes": (self.n - ns) * 4 * dim + sum(s.memory_bytes() for s in self.sparse.values())}


def vectors_from_csr(dimension, indptr, positions, values):
    indptr = [int(x) for x in indptr]
    return [SparseVector.from_parts(dimension, positions[a:b], values[a:b]) for a, b in zip(indptr[:-1], indptr[1:])]


def csr_of(svs):
    indptr = np.zeros(len(svs) + 1, dtype=np.uint64)
    indptr[1:] = np.cumsum([len(s) for s in svs])
    pos = np.array([p for s in svs for p in s.positions], dtype=np.uint32)
    val = np.concatenate([np.asarray(s.values, dtype=F) for s in svs]) if svs else np.zeros(0, dtype=F)
    return indptr, pos, val.astype(F)


def sparsify(rng, rows, zero_share):
    """rows with `zero_share` of the elements of each zeroed (at least one kept is not promised)"""
    rows = np.array(rows, dtype=F)
    mask = rng.random(rows.shape) < zero_share
    rows[mask] = 0.0
    return rows


def build_mixed(rows, sparse_mask, config=None):
    """rows[i] inserted Sparse(from_dense) where sparse_mask[i], Dense otherwise"""
    idx = HNSWMixedIndex(config)
    for r, s in zip(np.asarray(rows, dtype=F), sparse_mask):
        if s:
            idx.insert_sparse(SparseVector.from_dense(r))
        else:
            idx.insert(r)
    return idx


def padded(results, k):
    ids = np.full((len(results), k), np.uint64(0xFFFFFFFFFFFFFFFF), dtype=np.uint64)
    sc = np.full((len(results), k), -np.inf, dtype=F)
    cnt = np.zeros(len(results), dtype=np.uint32)
    for i, res in enumerate(results):
        cnt[i] = len(res)
        for j, (nid, s) in enumerate(res):
            ids[i, j] = nid
            sc[i, j] = s
    return ids, sc, cnt


def answers_dense(idx, queries, k, ef=None):
    Q = np.atleast_2d(np.asarray(queries, dtype=F))
    return padded([idx.search_with_ef(q, k, idx.config.ef_search if ef is None else ef) for q in Q], k)


def answers_sparse(idx, sqs, k, ef=None):
    return padded([idx.search_sparse_with_ef(s, k, idx.config.ef_search if ef is None else ef) for s in sqs], k)


# ---- tests/golden/hnsw_mixed_small.npz -----------------------------------------------------------------------------------------
def golden_corpus(n=400, dim=20, nq=64, seed=0x15A):
    """400 x 20; every second row is inserted Sparse with 70 % of its elements zeroed and the others doubled: under DotProduct the
    largest dots win, and rows that keep 30 % of their elements unscaled never reach a top 10 (measured: 6 of 64 queries saw one)"""
    rng = np.random.default_rng(seed)
    rows = rng.standard_normal((n, dim)).astype(F)
    mask = np.arange(n) % 2 == 1
    rows[mask] = sparsify(rng, rows[mask], 0.7) * F(2.0)
    queries = rng.standard_normal((nq, dim)).astype(F)
    return rows, mask, queries
