"""CPU restatement of the reference's extended distance metrics and of search_with_hnsw_and_metric — TEST INFRASTRUCTURE ONLY.

The product scores in neumann_amd/csrc/nmn_xmetric.hip (a HIP kernel); this file is written from the reference's text
independently of it (paths relative to the reference root):
  tensor_store/src/distance.rs       DistanceMetric 13-52, higher_is_better 60-69, compute 76-88, to_similarity 92-106,
                                     GeometricConfig 115-125, its presets 127-166, GeometricConfig::compute 172-193
  tensor_store/src/sparse_vector.rs  from_dense 221-229 (a value is stored iff `val != 0.0`: +-0.0 skipped, NaN stored),
                                     dot_f64 419-443, magnitude_f64 553-559, cosine_similarity 583-599, angular_distance
                                     795-798, geodesic_distance 805-808, jaccard_index 816-845, overlap_coefficient 852-878,
                                     weighted_jaccard 886-935, euclidean_distance 942-949 over euclidean_distance_squared_f64
                                     964-1006, manhattan_distance 1013-1059
  vector_engine/src/lib.rs           search_with_hnsw_and_metric 2560-2619

The sparse form is built as the reference builds it (positions and values of the stored entries) and every metric walks the two
position lists with the reference's merge loop.  Every f64 sum is an explicit left-to-right loop over Python floats (IEEE
doubles: each `+`, `*`, `-`, `/` rounds once), every f32 step is one np.float32 operation, and the fused `mul_add` goes through
exact rational arithmetic rounded once to f32.

Two points are restated from memory, because `std` is not part of the reference:
  * `f32::midpoint(a, b)` on x86-64 is `((a as f64 + b as f64) / 2.0) as f32` — one rounding.
  * `f32::acos` is the platform's libm, so the reference itself does not pin its bits.  Here (as in the product) it is acos in
    f64 of the f32 cosine, rounded once to f32: `np.float32(math.acos(float(cos32)))`.  Angular and Geodesic are therefore held
    to one ulp instead of bit equality.
`sort_by` is a stable sort (as list.sort); `partial_cmp(..).unwrap_or(Equal)` on NaN scores is not a parity case.
"""
import math
from fractions import Fraction

import numpy as np

from tests import _hnsw_oracle as ho

F = np.float32
F32_MAX = float(np.finfo(np.float32).max)
PI32 = F(3.14159274101257324)  # std::f32::consts::PI

(COSINE, ANGULAR, GEODESIC, JACCARD, OVERLAP, WEIGHTED_JACCARD, EUCLIDEAN, MANHATTAN, COMPOSITE) = range(9)
NAMES = ("Cosine", "Angular", "Geodesic", "Jaccard", "Overlap", "WeightedJaccard", "Euclidean", "Manhattan", "Composite")


class GeometricConfig:
    def __init__(self, cosine_weight=0.5, structural_weight=0.3, magnitude_weight=0.2):  # Default, distance.rs:127-135
        self.cosine_weight = F(cosine_weight)
        self.structural_weight = F(structural_weight)
        self.magnitude_weight = F(magnitude_weight)

    @staticmethod
    def default():
        return GeometricConfig()

    @staticmethod
    def angular_heavy():  # 140-146
        return GeometricConfig(0.8, 0.1, 0.1)

    @staticmethod
    def structural_heavy():  # 150-156
        return GeometricConfig(0.2, 0.7, 0.1)

    @staticmethod
    def conflict_detection():  # 160-166
        return GeometricConfig(0.4, 0.5, 0.1)

    def weights(self):
        return (self.cosine_weight, self.structural_weight, self.magnitude_weight)


class Metric:
    def __init__(self, kind, config=None):
        self.kind = kind
        self.config = config if kind == COMPOSITE else None
        if kind == COMPOSITE and config is None:
            self.config = GeometricConfig()

    def __repr__(self):
        return NAMES[self.kind]


class Sparse:
    """SparseVector::from_dense"""

    def __init__(self, dense):
        d = np.asarray(dense, dtype=F)
        self.dimension = d.size
        self.positions = []
        self.values = []
        for i, v in enumerate(d.tolist()):  # (tolist: the f32 values as Python floats, exactly)
            if v != 0.0:
                self.positions.append(i)
                self.values.append(v)


def _as_f32(x):
    """`x as f32` of an f64"""
    with np.errstate(over="ignore", invalid="ignore"):
        return F(x)


def dot_f64(a, b):
    result = 0.0
    i = j = 0
    while i < len(a.positions) and j < len(b.positions):
        if a.positions[i] == b.positions[j]:
            result += a.values[i] * b.values[j]
            i += 1
            j += 1
        elif a.positions[i] < b.positions[j]:
            i += 1
        else:
            j += 1
    return result


def magnitude_f64(a):
    s = 0.0
    for v in a.values:
        s += v * v
    return math.sqrt(s)


def cosine_similarity(a, b):
    dot = dot_f64(a, b)
    mag_a = magnitude_f64(a)
    mag_b = magnitude_f64(b)
    if mag_a == 0.0 or mag_b == 0.0:
        return F(0.0)
    den = mag_a * mag_b
    try:
        result = dot / den
    except ZeroDivisionError:  # (a product of two magnitudes that underflowed: IEEE gives NaN or an infinity)
        result = math.nan if (dot == 0.0 or dot != dot) else math.copysign(math.inf, dot)
    if result != result or abs(result) == math.inf:
        return F(0.0)
    return _as_f32(min(max(result, -1.0), 1.0))


def angular_distance(a, b):
    cos = cosine_similarity(a, b)
    cos = F(min(max(cos, F(-1.0)), F(1.0)))
    return F(math.acos(float(cos)))


def _intersection(a, b):
    n = 0
    i = j = 0
    while i < len(a.positions) and j < len(b.positions):
        if a.positions[i] == b.positions[j]:
            n += 1
            i += 1
            j += 1
        elif a.positions[i] < b.positions[j]:
            i += 1
        else:
            j += 1
    return n


def jaccard_index(a, b):
    if not a.positions and not b.positions:
        return F(1.0)
    if not a.positions or not b.positions:
        return F(0.0)
    inter = _intersection(a, b)
    union = len(a.positions) + len(b.positions) - inter
    return F(inter) / F(union)


def overlap_coefficient(a, b):
    if not a.positions or not b.positions:
        return F(0.0)
    inter = _intersection(a, b)
    return F(inter) / F(min(len(a.positions), len(b.positions)))


def _merge(a, b):
    """the union walk of weighted_jaccard / euclidean / manhattan: (a value or None, b value or None) in position order"""
    i = j = 0
    na, nb = len(a.positions), len(b.positions)
    while i < na or j < nb:
        if i >= na:
            yield None, b.values[j]
            j += 1
        elif j >= nb:
            yield a.values[i], None
            i += 1
        elif a.positions[i] == b.positions[j]:
            yield a.values[i], b.values[j]
            i += 1
            j += 1
        elif a.positions[i] < b.positions[j]:
            yield a.values[i], None
            i += 1
        else:
            yield None, b.values[j]
            j += 1


def weighted_jaccard(a, b):
    min_sum = 0.0
    max_sum = 0.0
    for x, y in _merge(a, b):
        a_val = abs(x) if x is not None else 0.0
        b_val = abs(y) if y is not None else 0.0
        min_sum += min(a_val, b_val)
        max_sum += max(a_val, b_val)
    if max_sum == 0.0:
        return F(1.0)
    return _as_f32(min_sum / max_sum)


def euclidean_distance(a, b):
    sum_sq = 0.0
    for x, y in _merge(a, b):
        if x is None:
            diff = -y
        elif y is None:
            diff = x
        else:
            diff = x - y
        sum_sq += diff * diff
    dist = math.sqrt(sum_sq)
    return F(F32_MAX) if dist > F32_MAX else _as_f32(dist)


def manhattan_distance(a, b):
    s = 0.0
    for x, y in _merge(a, b):
        if x is None:
            diff = abs(y)
        elif y is None:
            diff = abs(x)
        else:
            diff = abs(x - y)
        s += diff
    return F(F32_MAX) if s > F32_MAX else _as_f32(s)


def midpoint(a, b):
    return _as_f32((float(F(a)) + float(F(b))) / 2.0)


def _round_f32(fr):
    """an exact rational to the nearest f32 (ties to even): float(Fraction) rounds once to f64, which is not always the same"""
    if fr == 0:
        return F(0.0)
    sign = -1 if fr < 0 else 1
    fr = abs(fr)
    e = fr.numerator.bit_length() - fr.denominator.bit_length()
    if Fraction(2) ** e > fr:
        e -= 1
    e = max(e, -126)          # subnormals share the exponent of the smallest normal
    q = fr / (Fraction(2) ** (e - 23))  # units in the last place
    n = q.numerator // q.denominator
    rem = q - n
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and n % 2 == 1):
        n += 1
    val = Fraction(n) * (Fraction(2) ** (e - 23))
    if val > Fraction(F32_MAX):
        return F(sign * math.inf)
    return F(sign * float(val))  # (exact: val is an f32)


def mul_add(a, b, c):
    """f32::mul_add: a * b + c rounded once"""
    a, b, c = F(a), F(b), F(c)
    if not (np.isfinite(a) and np.isfinite(b) and np.isfinite(c)):
        with np.errstate(all="ignore"):
            return F(float(a) * float(b) + float(c))
    exact = Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c))
    if exact != 0:
        r = _round_f32(exact)
        return r if r != 0 else (F(-0.0) if exact < 0 else F(0.0))  # (underflow keeps the sign)
    # an exact zero: -0.0 only when the product and the addend are both negative zeros
    product_negative = bool(np.signbit(a)) != bool(np.signbit(b))
    if (a == 0 or b == 0) and product_negative and np.signbit(c):
        return F(-0.0)
    return F(0.0)


def composite(cfg, a, b):
    cw, sw, mw = cfg.weights()
    total_weight = F(F(cw + sw) + mw)
    if total_weight == 0.0:
        return F(0.0)
    cosine_sim = midpoint(cosine_similarity(a, b), F(1.0))
    jaccard_sim = jaccard_index(a, b)
    euclidean_dist = euclidean_distance(a, b)
    euclidean_sim = F(1.0) / F(F(1.0) + euclidean_dist)
    inner = mul_add(sw, jaccard_sim, F(mw * euclidean_sim))
    with np.errstate(all="ignore"):
        return F(mul_add(cw, cosine_sim, inner) / total_weight)


def compute(metric, a, b):
    """DistanceMetric::compute on two Sparse"""
    k = metric.kind
    if k == COSINE:
        return cosine_similarity(a, b)
    if k in (ANGULAR, GEODESIC):
        return angular_distance(a, b)
    if k == JACCARD:
        return jaccard_index(a, b)
    if k == OVERLAP:
        return overlap_coefficient(a, b)
    if k == WEIGHTED_JACCARD:
        return weighted_jaccard(a, b)
    if k == EUCLIDEAN:
        return euclidean_distance(a, b)
    if k == MANHATTAN:
        return manhattan_distance(a, b)
    return composite(metric.config, a, b)


def to_similarity(metric, raw):
    raw = F(raw)
    k = metric.kind
    if k == COSINE:
        return midpoint(raw, F(1.0))
    if k in (ANGULAR, GEODESIC):
        return F(F(1.0) - F(raw / PI32))
    if k in (EUCLIDEAN, MANHATTAN):
        with np.errstate(all="ignore"):
            return F(F(1.0) / F(F(1.0) + raw))
    return raw


def higher_is_better(metric):
    return metric.kind in (COSINE, JACCARD, OVERLAP, WEIGHTED_JACCARD, COMPOSITE)


def score_dense(metric, query, vector):
    """(compute, to_similarity(compute)) of two dense vectors; the shorter one is zero-padded (from_dense drops the zeros)"""
    q = np.asarray(query, dtype=F)
    v = np.asarray(vector, dtype=F)
    raw = compute(metric, Sparse(q), Sparse(v))
    return raw, to_similarity(metric, raw)


def score_matrix(metric, queries, rows):
    """raw and similarity, f32 [nq, n]"""
    Q = np.asarray(queries, dtype=F)
    R = np.asarray(rows, dtype=F)
    sq = [Sparse(q) for q in Q]
    sr = [Sparse(r) for r in R]
    raw = np.empty((len(sq), len(sr)), dtype=F)
    sim = np.empty_like(raw)
    for i, a in enumerate(sq):
        for j, b in enumerate(sr):
            raw[i, j] = compute(metric, a, b)
            sim[i, j] = to_similarity(metric, raw[i, j])
    return raw, sim


def candidate_count(top_k):
    return max(min(top_k * 2, (1 << 64) - 1), 10)  # top_k.saturating_mul(2).max(10)


def rerank(metric, query, candidates, vector_of, top_k):
    """lib.rs:2588-2617 on the walk's candidate ids: vector_of(id) -> (tag, vector) or None (dropped); -> [(tag, score f32)]"""
    qs = Sparse(query)
    results = []
    for nid in candidates:
        got = vector_of(nid)
        if got is None:
            continue
        tag, vec = got
        raw = compute(metric, qs, Sparse(vec))
        results.append((tag, to_similarity(metric, raw)))
    # sort_by(|a, b| b.score.partial_cmp(&a.score).unwrap_or(Equal)): stable, descending
    results.sort(key=lambda t: -float(t[1]))
    return results[:top_k]


def search_with_hnsw_and_metric(idx, key_mapping, current_vectors, query, top_k, metric):
    """lib.rs:2560-2619 -> [(key, score f32)].  idx: tests/_hnsw_oracle.py's HNSWIndex (its `search` is the walk);
    current_vectors: key -> vector, what get_embedding returns now."""
    if len(query) == 0:
        raise ValueError("Empty vector provided")
    if top_k == 0:
        raise ValueError("Invalid top_k value (must be > 0)")
    cands = [nid for nid, _ in idx.search(query, candidate_count(top_k))]

    def vector_of(nid):
        if nid >= len(key_mapping):
            return None
        key = key_mapping[nid]
        vec = current_vectors.get(key)
        return None if vec is None else (key, vec)

    return rerank(metric, query, cands, vector_of, top_k)


# ---- tests/golden/hnsw_small_sparse.npz (written by tests/golden/make_golden_hnsw_sparse.py) -------------------------------------
def sparse_golden_corpus():
    """_hnsw_oracle.golden_corpus() with 60 % of the entries of rows and queries zeroed: stored positions differ from row to row"""
    rows, queries = ho.golden_corpus()
    rng = np.random.default_rng(60)
    rows = rows.copy()
    queries = queries.copy()
    rows[rng.random(rows.shape) < 0.6] = 0.0
    queries[rng.random(queries.shape) < 0.6] = 0.0
    return rows, queries


def index_from_golden(path):
    """the oracle's HNSWIndex as a golden file records it (rows, levels, lists, entry point): no rebuild"""
    g = np.load(path)
    idx = ho.HNSWIndex()
    idx.n = g["rows"].shape[0]
    idx.rows = g["rows"].astype(F)
    idx.mags = np.array([ho.magnitude(r) for r in idx.rows], dtype=F)
    idx.levels = g["levels"].tolist()
    idx.neighbors = [[[] for _ in range(lv + 1)] for lv in idx.levels]
    for node in range(idx.n):
        idx.neighbors[node][0] = g["l0"][node, :g["l0cnt"][node]].tolist()
    at = 0
    for node, layer, cnt in g["up_head"].tolist():
        idx.neighbors[node][layer] = g["up_ids"][at:at + cnt].tolist()
        at += cnt
    idx.entry_point = int(g["entry_point"])
    idx.max_layer = int(g["max_layer"])
    return idx
