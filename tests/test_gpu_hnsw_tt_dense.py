"""nmn_hnsw_search_tt_dense / _insert_tt_dense / _insert_batch_tt (GpuHnsw.search_tt_dense / insert_tt_dense / insert_batch_tt):
HNSWIndex::search_tt, insert_tt and insert_batch_tt from dense vectors and a TTConfig (docs/hnsw.md §21) — ids and score BITS
against nmn_tt_decompose followed by nmn_hnsw_search_tt, against tests/_hnsw_tt_oracle.py walking the twin's trains, and against
nmn_hnsw_search where the decomposition is an Err."""
import functools

import numpy as np
import pytest

from tests import _hnsw_oracle as ho
from tests import _hnsw_q8_oracle as qo
from tests import _hnsw_tt_oracle as to
from tests import _tt_decompose_oracle as do

pytestmark = pytest.mark.gpu
F = np.float32
N = 300
SHAPES = {64: (4, 4, 4), 128: (4, 4, 8)}
KINDS = [("dense", ho.COSINE, 64), ("dense", ho.EUCLIDEAN, 128), ("q8", ho.COSINE, 128), ("q8", ho.EUCLIDEAN, 64)]


def bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


def assert_same(got, want):
    ig, sg, cg = got[:3]
    iw, sw, cw = want[:3]
    assert np.array_equal(cg, cw), (cg, cw)
    assert np.array_equal(ig, iw), np.argwhere(ig != iw)[:5]
    assert np.array_equal(bits(sg), bits(sw)), np.argwhere(bits(sg) != bits(sw))[:5]


def o_cfg(metric):
    return ho.HNSWConfig.high_speed().with_distance_metric(metric)


def g_cfg(metric):
    from neumann_amd import HNSWConfig
    return HNSWConfig.high_speed().with_distance_metric(metric)


@functools.lru_cache(maxsize=None)
def corpus(dim):
    rng = np.random.default_rng(0x7761 + dim)
    return (rng.standard_normal((N, dim)) + 2.0 * rng.standard_normal((6, dim))[rng.integers(0, 6, N)]).astype(F)


@functools.lru_cache(maxsize=None)
def queries(dim):
    """six random vectors and six rank-one tensors, interleaved"""
    rng = np.random.default_rng(0x7762 + dim)
    q = rng.standard_normal((12, dim)).astype(F)
    for i in range(1, 12, 2):
        q[i] = do.rank_one(rng, SHAPES[dim])
    return q


@functools.lru_cache(maxsize=None)
def oracle(kind, metric, dim):
    return (ho if kind == "dense" else qo).build(corpus(dim), o_cfg(metric))


def gpu_index(kind, metric, dim):
    from neumann_amd import GpuHnsw
    g = GpuHnsw(dim, g_cfg(metric), storage="quantized" if kind == "q8" else None)
    g.insert(corpus(dim))
    return g


def twin_trains(vectors, shape, r, t):
    out = []
    for v in vectors:
        ranks, cores = do.tt_decompose(v, shape, r, t)
        out.append(to.TTVector(list(shape), ranks, cores))
    return out


@pytest.mark.parametrize("kind,metric,dim", KINDS)
def test_search_tt_dense(kind, metric, dim):
    from neumann_amd import NeumannGpuError, TTConfig, tt
    shape, q, o = SHAPES[dim], queries(dim), oracle(kind, metric, dim)
    cfg = TTConfig(shape, 8, 1e-4)
    with gpu_index(kind, metric, dim) as g:
        # every decomposition Ok: decompose, then search_tt — and the oracle's walk of the twin's trains
        got = g.search_tt_dense(q, 10, cfg)
        assert_same(got, g.search_tt(tt.tt_decompose(q, cfg), 10))
        assert_same(got, to.answers_tt(o, twin_trains(q, shape, 8, 1e-4), 10))
        assert_same(g.search_tt_dense(q[3], 4, cfg), to.answers_tt(o, twin_trains(q[3:4], shape, 8, 1e-4), 4))
        # tolerance 0.9: the randoms fail (EmptyMatrix) and fall back to `search` under the handle's metric, the rank-ones walk
        loose = TTConfig(shape, 8, 0.9)
        status = [isinstance(x, tt.TTDecomposeError) for x in tt.tt_decompose(q, loose, return_status=True)]
        assert status == [i % 2 == 0 for i in range(12)]
        ids, sc, cnt, st = g.search_tt_dense(q, 10, loose, with_stats=True)
        assert_same((ids[0::2], sc[0::2], cnt[0::2]), g.search(q[0::2], 10))
        if kind == "dense":
            assert_same((ids[0::2], sc[0::2], cnt[0::2]), ho.padded_answers(o, q[0::2], 10))
        assert_same((ids[1::2], sc[1::2], cnt[1::2]), to.answers_tt(o, twin_trains(q[1::2], shape, 8, 0.9), 10))
        assert st.sweep == "graph" and st.rows_scanned > 0
        # the three argument errors are an Err for every query: a plain dense search
        for bad in (TTConfig(shape[:-1], 8, 1e-4), TTConfig(shape, 0, 1e-4)):
            assert_same(g.search_tt_dense(q, 10, bad), g.search(q, 10))
        with pytest.raises(NeumannGpuError):
            g.search_tt_dense(q[:, :-1], 10, cfg)              # not the index's dimension


def test_two_core_rank_zero_query_is_refused_by_name():
    from neumann_amd import NeumannGpuError, TTConfig
    rng = np.random.default_rng(0x7764)
    q = np.stack([do.rank_one(rng, (8, 8)), do.rank_one(rng, (8, 8)), rng.standard_normal(64).astype(F)])
    assert do.tt_decompose(q[0], (8, 8), 8, 0.9)[0] == [1, 1, 1] and do.tt_decompose(q[2], (8, 8), 8, 0.9)[0] == [1, 0, 1]
    with gpu_index("dense", ho.COSINE, 64) as g:
        ok = g.search_tt_dense(q[:2], 5, TTConfig((8, 8), 8, 0.9))
        assert ok[2].tolist() == [5, 5]
        with pytest.raises(NeumannGpuError, match="query 2: every rank must be >= 1"):
            g.search_tt_dense(q, 5, TTConfig((8, 8), 8, 0.9))


@pytest.mark.parametrize("metric", [ho.COSINE, ho.EUCLIDEAN])
def test_insert_tt_dense_and_batch_build_inserts_graph(metric):
    from neumann_amd import GpuHnsw, TTConfig
    rows, cfg = corpus(64)[:120], TTConfig((4, 4, 4), 8, 1e-4)
    o = ho.build(rows, o_cfg(metric))
    with GpuHnsw(64, g_cfg(metric)) as g, GpuHnsw(64, g_cfg(metric)) as plain:
        plain.insert(rows)
        assert g.insert_tt_dense(rows[0], cfg) == 0
        assert g.insert_batch_tt(rows[1:50], cfg).tolist() == list(range(1, 50))
        assert g.insert_batch_tt(rows[50:], cfg).tolist() == list(range(50, 120))
        assert g.insert_batch_tt(np.zeros((0, 64), dtype=F), cfg).size == 0
        assert len(g) == len(plain) == 120 and g.entry_point == o.entry_point and g.levels().tolist() == o.levels
        for node in range(120):
            assert np.array_equal(bits(g.get_vector(node)), bits(rows[node]))
            for layer in range(o.levels[node] + 1):
                assert g.neighbors(node, layer).tolist() == o.neighbors[node][layer], (node, layer)
        assert_same(g.search(queries(64), 10), plain.search(queries(64), 10))


def test_insert_failures_insert_nothing():
    from neumann_amd import GpuHnsw, NeumannGpuError, TTConfig
    rng = np.random.default_rng(0x7763)
    rows = np.stack([do.rank_one(rng, (4, 4, 4)) for _ in range(6)])
    bad = rows.copy()
    bad[4] = rng.standard_normal(64).astype(F)
    bad[5] = rng.standard_normal(64).astype(F)
    loose = TTConfig((4, 4, 4), 8, 0.9)
    with GpuHnsw(64, g_cfg(ho.COSINE)) as g:
        g.insert_batch_tt(rows, loose)
        assert len(g) == 6
        with pytest.raises(NeumannGpuError, match=r"Batch TT decomposition failed: Decompose\(EmptyMatrix\) \(vector 4\)"):
            g.insert_batch_tt(bad, loose)
        with pytest.raises(NeumannGpuError, match=r"^.*TT decomposition failed: Decompose\(EmptyMatrix\)$"):
            g.insert_tt_dense(bad[4], loose)
        with pytest.raises(NeumannGpuError, match=r"TT decomposition failed: ShapeMismatch \{ dim: 64, shape: \[4, 4\], product: 16 \}"):
            g.insert_tt_dense(rows[0], TTConfig((4, 4), 8, 1e-4))
        with pytest.raises(NeumannGpuError, match="Batch TT decomposition failed: InvalidRank"):
            g.insert_batch_tt(rows, TTConfig((4, 4, 4), 0, 1e-4))
        assert len(g) == 6
    with GpuHnsw(64, g_cfg(ho.COSINE), storage="quantized") as g:
        with pytest.raises(NeumannGpuError, match="dense handle"):
            g.insert_batch_tt(rows, loose)
        with pytest.raises(NeumannGpuError, match="dense handle"):
            g.insert_tt_dense(rows[0], loose)
        assert len(g) == 0
