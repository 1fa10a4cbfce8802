"""Corpus generators shared between test modules (numpy only): the f32-underflow rows of tests/test_gpu_underflow.py and the
all-identical shard of tests/test_gpu_edge_cases.py, which tests/_select_walk_cases.py runs through the three-level walk as well.
Every function draws from the generator it is given in a fixed order, so a caller's corpus depends on its seed alone."""
import numpy as np

F = np.float32
STRADDLE = (F(2.5e-23), F(4e-23))


def straddle_rows(rng, m, d):
    """m rows of +-2.5e-23 / +-4e-23 (squares subnormal: the stored magnitude is far below the true one)."""
    v = np.where(rng.random((m, d)) < 0.8, STRADDLE[0], STRADDLE[1]).astype(F)
    return (v * rng.choice(np.array([-1, 1], F), (m, d))).astype(F)


def straddle_corpus(rng, n, d, ties=400):
    """Every row tiny; `ties` near-ties of one row (one element swapped between 2.5e-23 and 4e-23) around the cut.
    -> (rows, the tied row ids)."""
    A = straddle_rows(rng, n, d)
    tie = rng.choice(n, ties, replace=False)
    A[tie] = A[tie[0]]
    cols = rng.integers(0, d, ties)
    A[tie, cols] = np.where(np.abs(A[tie, cols]) == STRADDLE[0], STRADDLE[1], STRADDLE[0]) * np.sign(A[tie, cols])
    return A.astype(F), tie


def tiny_rows_along(rng, q, m):
    """m straddle rows with the signs of q: tiny rows whose inflated cosines (> 1) belong at the top of q's answer."""
    return (np.abs(straddle_rows(rng, m, q.size)) * np.sign(q)).astype(F)


def identical_rows(n, d):
    """Every row the same, and a query: every row ties under every metric.  -> (rows, query)"""
    return np.tile(np.linspace(-1, 1, d, dtype=F), (n, 1)), np.linspace(1, 2, d, dtype=F)
