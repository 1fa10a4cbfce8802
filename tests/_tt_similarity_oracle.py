"""CPU restatement of the reference's comparisons of tensor-train vectors — TEST INFRASTRUCTURE ONLY.

Written from the reference's text, independently of the product (neumann_amd/csrc/nmn_tt.hip); paths relative to the reference root:
  tensor_compress/src/tensor_train.rs  TTCore::get 240-243, tt_dot_product 480-516, tt_cosine_similarity 522-532,
                                       tt_euclidean_distance 539-546, the three _batch forms 591-646 (tt_norm 440-474 is
                                       _hnsw_tt_oracle's)

tt_dot_product keeps ONE chain per (a_idx, b_idx) from +0.0 over k, then ia, then ib of
    sum = sum + ((gram[ia * r1b + ib] * A[ia, k, a_idx]) * B[ib, k, b_idx])
numpy carrying the (a_idx, b_idx) outputs side by side and, in `dot_many`, the targets of one rank vector side by side as well —
outputs the reference computes independently.  Every operation is one numpy float32 operation: rounded once, never fused.  The one
fused operation of the reference, (-2.0f32).mul_add(dot_ab, dot_aa + dot_bb), is _hnsw_q8_oracle.fma32: exact product, one rounding.
"""
import numpy as np

from tests import _hnsw_q8_oracle as qo
from tests import _hnsw_tt_oracle as to

F = np.float32
TINY = F(1e-10)   # the f32 nearest to 1e-10, as the literal in `norm_a < 1e-10` is
DOT, COSINE, EUCLIDEAN = 0, 1, 2
INCOMPATIBLE_SHAPES = "incompatible TT shapes for operation"   # Display of TTError::IncompatibleShapes
TTVector, random_tt, pack = to.TTVector, to.random_tt, to.pack


class TTError(Exception):
    pass


def dot_many(a, bs):
    """tt_dot_product(a, b) for every b of bs -> f32 [len(bs)]; bs share ONE rank vector"""
    for b in bs:
        if a.shape != b.shape:
            raise TTError(INCOMPATIBLE_SHAPES)
        assert b.ranks == bs[0].ranks
    T = len(bs)
    gram = np.ones((T, 1), dtype=F)                                  # gram = [1.0]
    with np.errstate(all="ignore"):
        for c, ca in enumerate(a.cores):
            cb = np.stack([b.cores[c] for b in bs])                  # [T][r1b][n][r2b]
            r1a, n, r2a = ca.shape
            r1b, r2b = cb.shape[1], cb.shape[3]
            s = np.zeros((T, r2a, r2b), dtype=F)                     # let mut sum = 0.0
            for k in range(n):
                for ia in range(r1a):
                    for ib in range(r1b):
                        g = gram[:, 0] if gram.shape[1] == 1 else gram[:, ia * r1b + ib]
                        ga = g[:, None] * ca[ia, k, :][None, :]      # g * core_a.get(ia, k, a_idx)        [T][r2a]
                        s = s + ga[:, :, None] * cb[:, ib, k, :][:, None, :]
            gram = s.reshape(T, r2a * r2b)
    return gram[:, 0].copy()


def tt_dot_product(a, b):
    return dot_many(a, [b])[0]


def finish(op, dot, dot_aa, dot_bb):
    """what tt_cosine_similarity / tt_euclidean_distance make of the three dots (scalars or arrays)"""
    dot, dot_aa, dot_bb = np.broadcast_arrays(np.asarray(dot, dtype=F), np.asarray(dot_aa, dtype=F), np.asarray(dot_bb, dtype=F))
    if op == DOT:
        return dot.copy()
    with np.errstate(all="ignore"):
        if op == COSINE:
            na, nb = np.sqrt(dot_aa), np.sqrt(dot_bb)                # tt_norm: sqrt of the self chain
            return np.where((na < TINY) | (nb < TINY), F(0.0), dot / (na * nb)).astype(F)   # a NaN norm is not < 1e-10
        sq = np.atleast_1d(qo.fma32(np.full(dot.shape, -2.0, dtype=F), dot, dot_aa + dot_bb)).reshape(dot.shape)
        # f32::max(self, other): when one operand is NaN the OTHER is returned — NaN.max(0.0) is 0.0, written out here because
        # np.maximum would propagate the NaN
        clamped = np.where(np.isnan(sq), F(0.0), np.where(sq > 0, sq, F(0.0))).astype(F)
        return np.sqrt(clamped)


def self_dot(t):
    return tt_dot_product(t, t)


def similarity(op, queries, targets, self_q=None, self_t=None):
    """-> f32 [nq][nt]: out[i][j] = the reference's function of (queries[i], targets[j])"""
    out = np.empty((len(queries), len(targets)), dtype=F)
    groups = {}
    for j, t in enumerate(targets):
        groups.setdefault(tuple(t.ranks), []).append(j)
    if op != DOT:
        self_q = np.asarray([self_dot(q) for q in queries], dtype=F) if self_q is None else self_q
        self_t = np.asarray([self_dot(t) for t in targets], dtype=F) if self_t is None else self_t
    for i, q in enumerate(queries):
        for js in groups.values():
            d = dot_many(q, [targets[j] for j in js])
            out[i, js] = d if op == DOT else finish(op, d, self_q[i], self_t[js])
    return out


def tt_cosine_similarity(a, b):
    return similarity(COSINE, [a], [b])[0, 0]


def tt_euclidean_distance(a, b):
    return similarity(EUCLIDEAN, [a], [b])[0, 0]


def batch(op, query, targets):
    """tt_dot_product_batch / tt_cosine_similarity_batch / tt_euclidean_distance_batch: collect::<Result<Vec<_>, _>>() — one target of
    another shape fails the whole call; the rayon split at 4 targets changes no value"""
    for t in targets:
        if t.shape != query.shape:
            raise TTError(INCOMPATIBLE_SHAPES)
    return similarity(op, [query], list(targets))[0]


# ---- tests/golden/tt_similarity_small.npz (written by tests/golden/make_golden_tt_similarity.py) ------------------------------------
GOLDEN_SHAPE, GOLDEN_SEED = [2, 2, 5], 0x5151
GOLDEN_Q_RANKS, GOLDEN_T_RANKS = [1, 2, 2, 1], [1, 2, 3, 1]


def golden_sets():
    """16 queries at ranks [1,2,2,1]; 24 targets, the odd ones at ranks [1,2,3,1]; Gaussian cores"""
    rng = np.random.default_rng(GOLDEN_SEED)
    qs = [random_tt(rng, GOLDEN_SHAPE, GOLDEN_Q_RANKS) for _ in range(16)]
    ts = [random_tt(rng, GOLDEN_SHAPE, GOLDEN_T_RANKS if j % 2 else GOLDEN_Q_RANKS) for j in range(24)]
    return qs, ts


def one_ulp_pairs(n=300, seed=0x1234):
    """n trains of shape [2,2,5], ranks [1,2,2,1], each with a copy in which one core element is moved one ulp up: the pairs whose
    squared Euclidean distance, fma(-2, dot_ab, dot_aa + dot_bb), comes out NEGATIVE before the clamp -> [(a, b, sq f32)]"""
    rng = np.random.default_rng(seed)
    found = []
    for _ in range(n):
        a = random_tt(rng, [2, 2, 5], [1, 2, 2, 1])
        cores = [c.copy() for c in a.cores]
        k = int(rng.integers(0, 3))
        flat = cores[k].reshape(-1)
        e = int(rng.integers(0, flat.size))
        flat[e] = np.nextafter(flat[e], F(np.inf))
        b = TTVector(a.shape, a.ranks, cores)
        sq = qo.fma32(F(-2.0), tt_dot_product(a, b), self_dot(a) + self_dot(b))
        if sq < 0:
            found.append((a, b, F(sq)))
    return found
