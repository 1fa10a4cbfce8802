"""The twin of the top-k search over a delta set (docs/delta.md §8).  The scores are the existing twin's, tests/_delta_oracle.py; the
key map and the order are restated here in numpy from their definitions (docs/exactness.md): score descending, row ascending, -0.0
and +0.0 equal, every NaN equal to every other NaN and below -inf.  Nothing here calls the library."""
import numpy as np

from tests import _delta_oracle as do

F = np.float32
NO_ROW = -1                       # UINT64_MAX read as int64
KEY_NAN = 1


def score_to_key(scores):
    """f32 -> u32, order-preserving: a NaN is 1 (below -inf, whose key is 0x007FFFFF), -0.0 is folded into +0.0, a negative score is
    the complement of its bits, any other score its bits with the sign bit set"""
    s = np.ascontiguousarray(scores, dtype=F)
    b = s.view(np.uint32).copy()
    b[(b << np.uint32(1)) == 0] = 0
    neg = (b & np.uint32(0x80000000)) != 0
    key = np.where(neg, ~b, b | np.uint32(0x80000000)).astype(np.uint32)
    key[np.isnan(s)] = KEY_NAN
    return key


def top_k(scores, k):
    """one query's scores [n] -> (rows int64 [k], scores f32 [k], count): the first min(k, n) rows by (key descending, row
    ascending), each with its own score bits; the unused slots hold NO_ROW and -inf"""
    scores = np.ascontiguousarray(scores, dtype=F)
    n = scores.shape[0]
    key = score_to_key(scores).astype(np.int64)
    order = np.lexsort((np.arange(n), -key))[:k]          # the last key of lexsort is the primary one
    rows = np.full(k, NO_ROW, dtype=np.int64)
    out = np.full(k, -np.inf, dtype=F)
    rows[:order.size] = order
    out.view(np.uint32)[:order.size] = scores.view(np.uint32)[order]
    return rows, out, min(k, n)


def top_k_all(scores, k):
    """scores [nq][n] -> (rows int64 [nq][k], scores f32 [nq][k], counts uint32 [nq])"""
    scores = np.asarray(scores, dtype=F)
    got = [top_k(row, k) for row in scores]
    return (np.stack([g[0] for g in got]).reshape(len(got), k), np.stack([g[1] for g in got]).reshape(len(got), k),
            np.asarray([g[2] for g in got], dtype=np.uint32))


def scores_of(reg, deltas, queries, metric):
    """the twin's dot_dense ("dot") or cosine_similarity_dense ("cosine") of every row with every query -> f32 [nq][n]"""
    queries = np.asarray(queries, dtype=F)
    if not deltas:
        return np.zeros((queries.shape[0], 0), dtype=F)
    return do.dot_dense_all(reg, deltas, queries) if metric == "dot" else do.cosine_dense_all(reg, deltas, queries)


def search(reg, deltas, queries, k, metric="dot"):
    return top_k_all(scores_of(reg, deltas, queries, metric), k)
