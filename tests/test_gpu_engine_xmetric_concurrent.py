"""VectorEngine.search_with_hnsw_and_metric from several threads on an unchanged engine — the fast path, nmn_hnsw_search_metric on
the index's own rows — with a different metric and top_k per thread: keys and score bits equal the sequential answers, and the
calls leave the handle in merged batches (docs/hnsw.md §12)."""
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
F = np.float32
THREADS, CALLS, N, D = 8, 12, 1500, 24
TOPS = (1, 10, 50, 100, 5, 6, 64, 200)


def test_concurrent_fast_path_callers_merge_and_get_their_sequential_answers():
    from neumann_amd import ExtendedDistanceMetric as M, GeometricConfig, engine, synth_rows
    rows, Q = synth_rows(0x5EED0041, 0, N, D), synth_rows(0x5EED0042, 0, THREADS * CALLS, D)
    m9 = [M(k) for k in range(8)] + [M.Composite(GeometricConfig(0.2, 0.7, 0.1))]
    eng = engine.VectorEngine()
    for i in range(N):
        eng.store_embedding(f"k{i:05d}", rows[i])
    index, key_mapping = eng.build_hnsw_index_default()
    jobs = [(Q[j], TOPS[(j % THREADS) % len(TOPS)], m9[(j % THREADS + 1) % 9]) for j in range(len(Q))]

    def ask(j):
        q, k, m = jobs[j]
        return [(r.key, F(r.score).tobytes()) for r in eng.search_with_hnsw_and_metric(index, key_mapping, q, k, m)]

    want = [ask(j) for j in range(len(jobs))]
    g = index.gpu()
    b0, c0 = g.coalesce_stats()
    got, errs = [None] * len(jobs), []
    start = threading.Barrier(THREADS)

    def work(t):
        try:
            start.wait()
            for j in range(t, len(jobs), THREADS):
                got[j] = ask(j)
        except Exception as e:  # noqa: BLE001 - reported below
            errs.append(e)

    th = [threading.Thread(target=work, args=(t,)) for t in range(THREADS)]
    for x in th:
        x.start()
    for x in th:
        x.join()
    assert not errs, errs
    for j in range(len(jobs)):
        assert got[j] == want[j], (j, jobs[j][1:])
        assert len(got[j]) == jobs[j][1]
    batches, calls = g.coalesce_stats()
    assert batches - b0 > 0 and calls - c0 >= 2 * (batches - b0), (batches - b0, calls - c0)
