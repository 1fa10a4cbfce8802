"""CPU restatement of the reference's HNSW index with HNSWStorageStrategy::Quantized — TEST INFRASTRUCTURE ONLY.

Written from the reference's text, independently of the product (neumann_amd/csrc/nmn_hnsw.hip); paths relative to the
reference root, all in tensor_store/src/hnsw.rs:
  ScalarQuantizedVector::from_dense 324-356 (min / max folds, scale 1.0 below f32::EPSILON, `.round()` = half AWAY from zero),
  dequantize 363-368 (`f32::from(q).mul_add(scale, min_val)`: one rounding), memory_bytes 381-383, magnitude_immutable 401-407,
  dot_dense 414-464, squared_magnitude 471-516, euclidean_distance_dense 522-527;
  EmbeddingStorage::cosine_distance_dense 1035-1045 (magnitude() of a Quantized row is magnitude_immutable; `== 0.0` rule),
  euclidean_distance_dense 1097, dot_product_distance_dense 1136-1138;
  insert_quantized 1711-1714; try_insert_embedding's query `nodes[node_id].embedding.to_dense()` 1985 (= dequantize());
  the (Quantized, Quantized) arms of try_cosine / euclidean / dot_product_distance 2489-2500, 2585-2589, 2662-2666: both rows
  dequantized, then the dense simd::* functions.

So the index is the dense oracle over the DEQUANTIZED rows — its `_dist_pairs` is the pruning side as it stands — with
`_dist_query`, the query side of search_layer* at search and insert time, replaced by the quantized formulas.

`mul_add` must round once.  fma32 computes a * b exactly in f64 (48 significant bits), adds c in f64 rounded TO ODD (the
round-to-nearest sum corrected by the sign of its exact error, from the two-sum), and rounds that to f32: 53 >= 2 * 24 + 2 bits,
so the double rounding is innocuous.  tests/test_hnsw_q8_oracle_cpu.py holds it to exact rational arithmetic.
"""
import numpy as np

from tests import _hnsw_oracle as ho

F = np.float32
D = np.float64
EPSILON = F(1.1920929e-07)  # f32::EPSILON = 2^-23


def fma32(a, b, c):
    """a * b + c with ONE rounding to f32, elementwise (f32::mul_add)."""
    a = np.asarray(a, dtype=F).astype(D)
    b = np.asarray(b, dtype=F).astype(D)
    c = np.asarray(c, dtype=F).astype(D)
    p = a * b                       # exact
    s = p + c                       # round to nearest even
    bb = s - p                      # two-sum: s + err == p + c exactly
    err = (p - (s - bb)) + (c - bb)
    s, err = np.atleast_1d(s).copy(), np.atleast_1d(err)
    odd = (s.view(np.int64) & 1) != 0
    fix = (err != 0) & ~odd         # inexact and even: the odd neighbour on the side of the true value
    s[fix] = np.nextafter(s[fix], np.where(err[fix] > 0, np.inf, -np.inf))
    out = s.astype(F)
    return out.reshape(np.shape(p)) if np.ndim(p) else out[0]


def round_half_away(x):
    """f32::round: to the nearest integer, halves away from zero (x - trunc(x) is exact)"""
    x = np.asarray(x, dtype=F)
    t = np.trunc(x)
    return np.where(np.abs(x - t) >= F(0.5), t + np.copysign(F(1.0), x), t).astype(F)


def from_dense(v):
    """-> (codes u8, scale f32, min_val f32)"""
    v = np.asarray(v, dtype=F)
    mn, mx = F(np.inf), F(-np.inf)
    for x in v:                     # the folds (NaN is not a parity case)
        mn = x if x < mn else mn
        mx = x if x > mx else mx
    rng = F(mx - mn)
    scale = F(1.0) if abs(rng) < EPSILON else F(rng / F(255.0))
    r = round_half_away((v - mn) / scale)
    return np.clip(r, F(0.0), F(255.0)).astype(np.uint8), scale, F(mn)


def dequantize(codes, scale, min_val):
    return fma32(np.asarray(codes).astype(F), F(scale), F(min_val))


def _chains(T):
    """terms [r][dim] -> for every row: eight accumulator chains over the whole chunks of eight (chain l takes the terms 8c + l in
    ascending c, from +0.0), the chains summed left to right from -0.0, then the remaining terms one by one"""
    T = np.asarray(T, dtype=F)
    r, dim = T.shape
    chunks = dim // 8
    acc = np.zeros((r, 8), dtype=F)
    for c in range(chunks):
        acc = acc + T[:, 8 * c:8 * c + 8]
    res = np.full(r, -0.0, dtype=F)
    for lane in range(8):
        res = res + acc[:, lane]
    for i in range(chunks * 8, dim):
        res = res + T[:, i]
    return res


def dot_dense(codes, scale, min_val, y, sum_y=None):
    """rows of codes [r][dim] (scale, min_val per row) against one dense vector"""
    C = np.atleast_2d(codes).astype(F)
    y = np.asarray(y, dtype=F)
    if sum_y is None:
        sum_y = _chains(y[None, :])[0]
    q_dot_y = _chains(C * y)                             # product and sum rounded separately
    return fma32(scale, q_dot_y, np.asarray(min_val, dtype=F) * F(sum_y))


def squared_magnitude(codes, scale, min_val):
    C = np.atleast_2d(codes).astype(F)
    scale = np.asarray(scale, dtype=F)
    min_val = np.asarray(min_val, dtype=F)
    sum_q_sq = _chains(C * C)
    sum_q = _chains(C)
    n = F(C.shape[1])
    scale_sq = scale * scale
    min_sq = min_val * min_val
    inner = fma32((F(2.0) * scale) * min_val, sum_q, min_sq * n)
    return fma32(scale_sq, sum_q_sq, inner)


def euclidean_distance_dense(codes, scale, min_val, y, x_sq=None, sum_y=None, y_sq=None):
    y = np.asarray(y, dtype=F)
    if x_sq is None:
        x_sq = squared_magnitude(codes, scale, min_val)
    if y_sq is None:
        y_sq = ho.dot_product_rows(y[None, :], y)[0]     # simd::sum_of_squares
    dot = dot_dense(codes, scale, min_val, y, sum_y)
    t = fma32(F(2.0), -dot, np.asarray(x_sq, dtype=F) + F(y_sq))
    return np.sqrt(np.maximum(t, F(0.0)))


class HNSWQ8Index(ho.HNSWIndex):
    def __init__(self, config=None):
        super().__init__(config)
        self.codes = None          # [capacity][dim] u8
        self.scale = None
        self.min_val = None
        self.x_sq = None           # squared_magnitude() of every row
        self._qside = (None, None, None)

    # insert_quantized: from_dense, then try_insert_embedding, whose query is the node's own to_dense()
    def insert(self, vector):
        codes, scale, mn = from_dense(vector)
        node_id = self.n
        if self.codes is None:
            self.codes = np.zeros((64, codes.size), dtype=np.uint8)
            self.scale = np.zeros(64, dtype=F)
            self.min_val = np.zeros(64, dtype=F)
            self.x_sq = np.zeros(64, dtype=F)
        if node_id == self.codes.shape[0]:
            self.codes = np.concatenate([self.codes, np.zeros_like(self.codes)])
            self.scale = np.concatenate([self.scale, np.zeros_like(self.scale)])
            self.min_val = np.concatenate([self.min_val, np.zeros_like(self.min_val)])
            self.x_sq = np.concatenate([self.x_sq, np.zeros_like(self.x_sq)])
        self.codes[node_id] = codes
        self.scale[node_id] = scale
        self.min_val[node_id] = mn
        self.x_sq[node_id] = squared_magnitude(codes, scale, mn)[0]
        return super().insert(dequantize(codes, scale, mn))

    def _query_side(self, q):
        """(sum_y, y_sq): they depend on the query alone"""
        if self._qside[0] is not q:
            q32 = np.asarray(q, dtype=F)
            self._qside = (q, _chains(q32[None, :])[0], ho.dot_product_rows(q32[None, :], q32)[0])
        return self._qside[1], self._qside[2]

    # EmbeddingStorage::distance_dense(Quantized rows `ids`, query)
    def _dist_query(self, ids, q, qmag):
        metric = self.config.distance_metric
        ids = np.asarray(ids, dtype=np.int64)
        self.distance_evals += len(ids)
        sum_y, y_sq = self._query_side(q)
        C, sc, mn = self.codes[ids], self.scale[ids], self.min_val[ids]
        if metric == ho.EUCLIDEAN:
            return euclidean_distance_dense(C, sc, mn, q, self.x_sq[ids], sum_y, y_sq)
        dot = dot_dense(C, sc, mn, q, sum_y)
        if metric == ho.DOT_PRODUCT:
            return -dot
        mag_self = self.mags[ids]                        # magnitude_immutable: simd::magnitude(dequantize())
        with np.errstate(divide="ignore", invalid="ignore"):
            d = F(1.0) - (dot / (mag_self * qmag))
        d[(mag_self == 0) | (qmag == 0)] = F(1.0)
        return d

    def get_vector(self, node):
        return dequantize(self.codes[node], self.scale[node], self.min_val[node])

    def memory_bytes(self):
        return self.n * (16 + self.codes.shape[1]) if self.n else 0


def build(rows, config=None):
    idx = HNSWQ8Index(config)
    for r in np.asarray(rows, dtype=F):
        idx.insert(r)
    return idx


# ---- tests/golden/hnsw_q8_small.npz (written by tests/golden/make_golden_hnsw_q8.py) ------------------------------------------
GOLDEN_K, GOLDEN_EF2 = 10, 120
