"""CPU restatement of the reference's HNSW search with a SPARSE query — TEST INFRASTRUCTURE ONLY.

Written from the reference's text, independently of the product (neumann_amd/csrc/nmn_hnsw.hip); paths relative to the
reference root:
  tensor_store/src/sparse_vector.rs  try_from_parts 155-193 (a position >= dimension is an error; `val != 0.0` keeps NaN and drops
                                     both zeros; `sort_by_key` on the position is stable, so duplicates survive in input order),
                                     try_from_dense 212-236, to_dense 400-406 (entries written in order: the last of a position
                                     wins), dot_dense 450-466 (`Iterator::sum::<f64>()` of f64(val) * f64(dense[pos]), `as f32`),
                                     magnitude 548-559 (the same sum over f64(v) * f64(v), f64 sqrt, `as f32`)
  tensor_store/src/hnsw.rs           try_dot_with_sparse 879-900 (Dense: query.dot_dense(v); Quantized: q.dot_dense(&query.to_dense())),
                                     try_magnitude 971-986, cosine_distance_sparse 1069-1079, euclidean_distance_sparse 1108-1114
                                     (simd::euclidean_distance(v, query.to_dense()); Quantized 1121-1124), dot_product_distance_sparse
                                     1143-1145, distance_sparse 1175-1181, search_sparse 2060-2062, search_sparse_with_ef 2118-2166,
                                     search_layer_greedy_sparse 2204-2234, search_layer_sparse 2339-2393

The walk is the dense one (ef.max(k), both heaps, should_add, the trimming, the strict termination test, the stable sort,
to_similarity) with distance_sparse in place of distance_dense, so it runs over the existing oracle indexes: a shallow copy of
`_hnsw_oracle.HNSWIndex` or `_hnsw_q8_oracle.HNSWQ8Index` whose distance and query-magnitude hooks are overridden.

std's float `Sum` is restated as the project restates it for simd::dot_product's lane sum: a left-to-right fold from -0.0
(docs/hnsw.md §1).  It shows only for a query with no stored entry.  A product of two f32 is exact in f64 (48 significant bits),
every addition rounds once, the cast rounds once: Python floats ARE f64, numpy's float64 -> float32 conversion rounds to nearest
even.
"""
import math

import numpy as np

from tests import _hnsw_oracle as ho
from tests import _hnsw_q8_oracle as q8

F = np.float32
D = np.float64


class IndexOutOfBounds(Exception):
    def __init__(self, index, dimension):
        super().__init__(f"index {index} out of bounds for dimension {dimension}")
        self.index, self.dimension = index, dimension


class SparseQuery:
    def __init__(self, dimension, positions, values):
        self.dimension = int(dimension)
        self.positions = [int(p) for p in positions]
        self.values = np.asarray(values, dtype=F).reshape(-1)

    @classmethod
    def from_parts(cls, dimension, positions, values):
        values = np.asarray(values, dtype=F).reshape(-1)
        pairs = []
        for pos, val in zip(positions, values):
            if int(pos) >= dimension:
                raise IndexOutOfBounds(int(pos), dimension)
            if val != 0.0:            # NaN != 0.0 is true: kept; +0.0 and -0.0 are dropped
                pairs.append((int(pos), val))
        pairs.sort(key=lambda t: t[0])  # stable
        return cls(dimension, [p for p, _ in pairs], [v for _, v in pairs])

    @classmethod
    def from_dense(cls, dense):
        dense = np.asarray(dense, dtype=F).reshape(-1)
        keep = [i for i, v in enumerate(dense) if v != 0.0]
        return cls(dense.size, keep, dense[keep])

    def __len__(self):
        return len(self.positions)

    def to_dense(self):
        out = np.zeros(self.dimension, dtype=F)
        for pos, val in zip(self.positions, self.values):
            out[pos] = val
        return out

    def dot_dense_rows(self, A):
        """dot_dense against every row of A [r][dimension] -> f32 [r]"""
        A = np.asarray(A, dtype=F)
        acc = np.full(A.shape[0], -0.0, dtype=D)
        for pos, val in zip(self.positions, self.values):
            acc = acc + D(val) * A[:, pos].astype(D)
        return acc.astype(F)

    def dot_dense(self, dense):
        return self.dot_dense_rows(np.asarray(dense, dtype=F)[None, :])[0]

    def magnitude(self):
        acc = -0.0
        for val in self.values:
            acc = acc + float(val) * float(val)
        return F(math.sqrt(acc))


class _SparseOnDense(ho.HNSWIndex):
    """distance_sparse on Dense rows: Cosine / DotProduct through dot_dense, Euclidean through to_dense (q IS to_dense)."""

    def _qmag(self, q):
        return self._sq.magnitude() if self.config.distance_metric == ho.COSINE else F(0)

    def _dist_query(self, ids, q, qmag):
        metric = self.config.distance_metric
        if metric == ho.EUCLIDEAN:
            return super()._dist_query(ids, q, qmag)
        self.distance_evals += len(ids)
        dot = self._sq.dot_dense_rows(self.rows[ids])
        if metric == ho.DOT_PRODUCT:
            return -dot
        mag_self = self.mags[ids]
        with np.errstate(divide="ignore", invalid="ignore"):
            d = F(1.0) - (dot / (mag_self * F(qmag)))
        d[(mag_self == 0) | (qmag == 0)] = F(1.0)
        return d


class _SparseOnQ8(q8.HNSWQ8Index):
    """distance_sparse on Quantized rows: every dot is q.dot_dense(&Q.to_dense()), so only Cosine's query magnitude changes."""

    def _qmag(self, q):
        return self._sq.magnitude() if self.config.distance_metric == ho.COSINE else F(0)


def _walker(idx, sq):
    cls = _SparseOnQ8 if isinstance(idx, q8.HNSWQ8Index) else _SparseOnDense
    w = cls.__new__(cls)
    w.__dict__.update(idx.__dict__)   # rows, graph and config are shared, never written by a search
    w._sq = sq
    w.distance_evals = 0
    if cls is _SparseOnQ8:
        w._qside = (None, None, None)
    return w


def search_sparse_with_ef(idx, sq, k, ef, evals=None):
    """-> [(id, similarity f32)]; `evals`, a list, receives the number of distance evaluations"""
    if sq.dimension != (idx.rows.shape[1] if idx.rows is not None else sq.dimension):
        raise ValueError("dimension mismatch")
    w = _walker(idx, sq)
    res = w.search_with_ef(sq.to_dense(), k, ef)
    if evals is not None:
        evals.append(w.distance_evals)
    return res


def search_sparse(idx, sq, k):
    return search_sparse_with_ef(idx, sq, k, idx.config.ef_search)


def queries_from_csr(dimension, indptr, positions, values):
    indptr = [int(x) for x in indptr]
    return [SparseQuery.from_parts(dimension, positions[a:b], values[a:b]) for a, b in zip(indptr[:-1], indptr[1:])]


def csr_from_dense(queries):
    """SparseVector::from_dense row by row, as CSR"""
    Q = np.atleast_2d(np.asarray(queries, dtype=F))
    sqs = [SparseQuery.from_dense(q) for q in Q]
    indptr = np.zeros(len(sqs) + 1, dtype=np.uint64)
    indptr[1:] = np.cumsum([len(s) for s in sqs])
    pos = np.array([p for s in sqs for p in s.positions], dtype=np.uint32)
    val = np.concatenate([s.values for s in sqs]) if sqs else np.zeros(0, dtype=F)
    return indptr, pos, val.astype(F)


def padded_answers(idx, sqs, k, ef=None):
    """the library's output layout and the evaluations made: (ids u64 [nq][k], scores f32, counts u32), evals"""
    ids = np.full((len(sqs), k), np.uint64(0xFFFFFFFFFFFFFFFF), dtype=np.uint64)
    sc = np.full((len(sqs), k), -np.inf, dtype=F)
    cnt = np.zeros(len(sqs), dtype=np.uint32)
    evals = []
    for i, sq in enumerate(sqs):
        res = search_sparse_with_ef(idx, sq, k, idx.config.ef_search if ef is None else ef, evals)
        cnt[i] = len(res)
        for j, (nid, s) in enumerate(res):
            ids[i, j] = nid
            sc[i, j] = s
    return (ids, sc, cnt), int(sum(evals))
