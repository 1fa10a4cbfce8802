"""HNSWStorageStrategy::Quantized on the GPU (nmn_hnsw_create_with_storage, GpuHnsw(..., storage="quantized")) against
tests/_hnsw_q8_oracle.py: every code, scale, min and dequantized bit of every row, the graph nmn_hnsw_insert builds, and every
answer of nmn_hnsw_search / nmn_hnsw_search_device — ids exact, score BITS equal, every query compared in full."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import _hnsw_oracle as ho
from tests import _hnsw_q8_oracle as q8

pytestmark = pytest.mark.gpu
F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "hnsw_q8_small.npz")
METRICS = [ho.COSINE, ho.EUCLIDEAN, ho.DOT_PRODUCT]
SEARCHES = ((1, 0), (10, 50), (25, 10))          # (k, ef), ef 0 = ef_search; (n + 5, 0) is added per corpus


def o_cfg(preset, metric):
    c = {"default": ho.HNSWConfig, "high_recall": ho.HNSWConfig.high_recall, "high_speed": ho.HNSWConfig.high_speed}[preset]()
    return c.with_distance_metric(metric)


def g_cfg(preset, metric):
    from neumann_amd import HNSWConfig
    return getattr(HNSWConfig, preset)().with_distance_metric(metric)


@functools.lru_cache(maxsize=None)
def corpus(name):
    """name -> (rows, queries); the generators of tests/test_gpu_hnsw.py, and `halves`"""
    rng = np.random.default_rng(sum(map(ord, name)))
    kind, n, d = name.split(":")
    n, d = int(n), int(d)
    rows = (rng.standard_normal((n, d)) + 2.0 * rng.standard_normal((6, d))[rng.integers(0, 6, n)]).astype(F)
    if kind == "dup":      # a quarter of the rows are exact duplicates of earlier ones
        for i in range(4, n, 4):
            rows[i] = rows[rng.integers(0, i)]
    elif kind == "same":   # identical rows only
        rows[:] = rows[0]
    elif kind == "zeros":  # some zero rows (scale 1.0; the distance 1.0 rule under Cosine)
        rows[::7] = 0.0
    elif kind == "halves":  # elements from {0, 0.5, .., 255}, element 0 = 0.0 and element 1 = 255.0: scale is exactly 1.0, every x.5
        rows = (rng.integers(0, 511, (n, d)) * 0.5).astype(F)  # meets the rounding rule, and integer-like codes tie distances
        rows[:, 0], rows[:, 1] = 0.0, 255.0
    queries = rng.standard_normal((40, d)).astype(F)
    if kind == "halves":
        queries = (rng.integers(0, 511, (40, d)) * 0.5).astype(F)
    queries[:10] = rows[rng.integers(0, n, 10)]
    if kind == "zeros":
        queries[10] = 0.0
    return rows, queries


@functools.lru_cache(maxsize=None)
def oracle(name, preset, metric):
    return q8.build(corpus(name)[0], o_cfg(preset, metric))


def gpu_index(name, preset, metric, batches=None, **kw):
    from neumann_amd import GpuHnsw
    rows = corpus(name)[0]
    g = GpuHnsw(rows.shape[1], g_cfg(preset, metric), storage="quantized", **kw)
    at = 0
    for b in batches or [len(rows)]:
        got = g.insert(rows[at:at + b])
        assert got.tolist() == list(range(at, min(at + b, len(rows))))
        at += b
    assert at >= len(rows) and len(g) == len(rows)
    return g


def assert_graph(g, o):
    assert len(g) == len(o)
    assert g.entry_point == o.entry_point and g.max_layer == o.max_layer
    assert g.levels().tolist() == o.levels
    for node in range(len(o)):
        for layer in range(o.levels[node] + 1):
            assert g.neighbors(node, layer).tolist() == o.neighbors[node][layer], (node, layer)
        assert g.neighbors(node, o.levels[node] + 1).size == 0


def assert_rows(g, o):
    """every code, scale, min and get_vector bit of every row"""
    for node in range(len(o)):
        codes, scale, mn = g.quantized_row(node)
        assert np.array_equal(codes, o.codes[node]), node
        assert scale.tobytes() == o.scale[node].tobytes() and mn.tobytes() == o.min_val[node].tobytes(), node
        assert g.get_vector(node).tobytes() == o.rows[node].tobytes() == o.get_vector(node).tobytes(), node


def assert_same(got, want):
    ig, sg, cg = got[:3]
    iw, sw, cw = want
    assert np.array_equal(cg, cw), (cg, cw)
    assert np.array_equal(ig, iw), np.argwhere(ig != iw)[:5]
    assert np.array_equal(np.ascontiguousarray(sg).view(np.uint32), np.ascontiguousarray(sw).view(np.uint32))


def dev(Q):
    import torch
    return torch.from_numpy(np.ascontiguousarray(np.atleast_2d(Q), dtype=F)).cuda()


def host(res):
    ids, sc, counts = res
    return ids.cpu().numpy().view(np.uint64), sc.cpu().numpy(), counts.cpu().numpy().astype(np.uint32)


def want_answers(o, Q, k, ef):
    """(ids, scores, counts), evaluations the oracle made"""
    o.distance_evals = 0
    res = ho.padded_answers(o, Q, k, ef or None)
    return res, o.distance_evals


def check_searches(g, o, Q, searches, device=True):
    import torch
    for k, ef in searches:
        want, evals = want_answers(o, Q, k, ef)
        ids, sc, cnt, st = g.search(Q, k, ef or None, with_stats=True)
        assert_same((ids, sc, cnt), want)
        assert st.sweep == "graph" and st.rows_scanned == evals, (k, ef, st.rows_scanned, evals)
        if device:
            got = g.search_device(dev(Q), k, ef or None)
            torch.cuda.synchronize()
            assert_same(host(got), want)


# ---- the graph and the rows ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("preset", ["default", "high_speed"])
@pytest.mark.parametrize("metric", METRICS)
def test_graph_and_rows_equal_oracle(metric, preset):
    name = "plain:360:20"
    o = oracle(name, preset, metric)
    Q = corpus(name)[1]
    with gpu_index(name, preset, metric) as g:
        assert g.storage == "quantized"
        assert_graph(g, o)
        assert_rows(g, o)
        check_searches(g, o, Q, SEARCHES + ((365, 0),))
    with gpu_index(name, preset, metric, batches=[1, 7, 352]) as g:      # inserts in batches: the same graph, the same answers
        assert_graph(g, o)
        check_searches(g, o, Q, ((10, 50),), device=False)


def test_golden_file():
    from neumann_amd import GpuHnsw, HNSWConfig
    z = np.load(GOLDEN)
    m, m0, efc, efs, metric = z["config"].tolist()
    cfg = HNSWConfig(m=m, m0=m0, ef_construction=efc, ef_search=efs, distance_metric=metric)
    with GpuHnsw(z["rows"].shape[1], cfg, storage="quantized") as g:
        g.insert(z["rows"])
        for node in range(len(g)):
            codes, scale, mn = g.quantized_row(node)
            assert np.array_equal(codes, z["codes"][node]) and scale.tobytes() == z["scale"][node].tobytes()
            assert mn.tobytes() == z["min_val"][node].tobytes() and g.get_vector(node).tobytes() == z["dequantized"][node].tobytes()
        assert g.levels().tolist() == z["levels"].tolist()
        assert g.entry_point == int(z["entry_point"]) and g.max_layer == int(z["max_layer"])
        for node in range(len(g)):
            c = int(z["l0cnt"][node])
            assert g.neighbors(node, 0).tolist() == z["l0"][node, :c].tolist()
        at = 0
        for node, layer, c in z["up_head"].tolist():
            assert g.neighbors(node, layer).tolist() == z["up_ids"][at:at + c].tolist()
            at += c
        k = int(z["k"])
        assert_same(g.search(z["queries"], k), (z["ids"], z["scores"], z["counts"]))
        assert_same(g.search(z["queries"], k, int(z["ef2"])), (z["ids_ef2"], z["scores_ef2"], z["counts_ef2"]))


# ---- chunking: no whole chunk, whole chunks only, tails, half a 16-byte load, many loads ------------------------------------------------
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("dim", [5, 8, 20, 24, 33, 128, 771])
def test_dimensions(dim, metric):
    name = f"plain:200:{dim}"
    o = oracle(name, "high_speed", metric)
    Q = corpus(name)[1]
    with gpu_index(name, "high_speed", metric) as g:
        assert_graph(g, o)
        assert_rows(g, o)
        check_searches(g, o, Q, ((10, 50), (205, 0)))


# ---- corpora that exercise the rules ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("name", ["dup:400:16", "same:150:9", "zeros:200:12", "halves:300:16"])
def test_corpora(name, metric):
    o = oracle(name, "high_speed", metric)
    rows, Q = corpus(name)
    with gpu_index(name, "high_speed", metric) as g:
        assert_graph(g, o)
        assert_rows(g, o)
        check_searches(g, o, Q, SEARCHES + ((len(rows) + 5, 0),))
    if name.startswith("halves"):
        assert np.all(o.scale[:o.n] == F(1.0)) and np.all(o.min_val[:o.n] == F(0.0))
        halves = rows != np.floor(rows)
        assert halves.any() and np.array_equal(o.codes[:o.n][halves], (np.floor(rows[halves]) + 1).astype(np.uint8))  # x.5 -> x + 1
    if name.startswith("zeros"):
        assert o.scale[0] == F(1.0) and not o.codes[0].any()
        if metric == ho.COSINE:   # a zero row and a zero query: distance 1.0, similarity 0.0
            (_, sc, cnt), _ = want_answers(o, Q[10], 5, 0)
            assert cnt[0] == 5 and np.all(sc[0] == 0.0)


# ---- both overflow paths ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", METRICS)
def test_lds_heap_overflow_goes_to_the_spill_launch(metric):
    import torch
    name = "plain:360:20"
    o = oracle(name, "high_speed", metric)
    Q = corpus(name)[1]
    want, evals = want_answers(o, Q, 10, 50)
    with gpu_index(name, "high_speed", metric) as g:
        g.set_heap_capacity(candidates=8)
        ids, sc, cnt, st = g.search(Q, 10, 50, with_stats=True)
        assert_same((ids, sc, cnt), want)
        assert st.fallback_queries > 0 and st.rows_scanned == evals
        got = g.search_device(dev(Q), 10, 50)
        torch.cuda.synchronize()
        assert_same(host(got), want)
        g.set_heap_capacity(results=16)
        ids, sc, cnt, st = g.search(Q, 10, 50, with_stats=True)
        assert_same((ids, sc, cnt), want)
        assert st.fallback_queries == len(Q)
        g.set_heap_capacity()
        ids, sc, cnt, st = g.search(Q, 10, 50, with_stats=True)
        assert_same((ids, sc, cnt), want)
        assert st.fallback_queries == 0


def test_ef_above_the_lds_results_heap():
    """ef 1100 on 1500 x 8: more results than a wave keeps in LDS, every query goes to the spill launch"""
    name = "plain:1500:8"
    o = oracle(name, "high_speed", ho.EUCLIDEAN)
    Q = corpus(name)[1]
    want, evals = want_answers(o, Q, 10, 1100)
    with gpu_index(name, "high_speed", ho.EUCLIDEAN) as g:
        ids, sc, cnt, st = g.search(Q, 10, 1100, with_stats=True)
        assert_same((ids, sc, cnt), want)
        assert st.fallback_queries == len(Q) and st.rows_scanned == evals


def test_host_search_env_in_child_process(tmp_path):
    """NMN_HNSW_HOST_SEARCH=1 (the walk on the host, the code insertion uses) in a fresh child process: the same bits"""
    name = "dup:400:16"
    rows, Q = corpus(name)
    np.save(tmp_path / "rows.npy", rows)
    np.save(tmp_path / "q.npy", Q)
    code = (
        "import sys, numpy as np\n"
        f"sys.path.insert(0, {ROOT!r})\n"
        "from neumann_amd import GpuHnsw, HNSWConfig\n"
        f"d = {str(tmp_path)!r}\n"
        "rows, Q = np.load(d + '/rows.npy'), np.load(d + '/q.npy')\n"
        "for metric in (0, 1, 2):\n"
        "    with GpuHnsw(rows.shape[1], HNSWConfig.high_speed().with_distance_metric(metric), storage='quantized') as g:\n"
        "        g.insert(rows)\n"
        "        ids, sc, cnt, st = g.search(Q, 10, with_stats=True)\n"
        "        assert st.sweep_launches == 0, st.sweep_launches\n"
        "        np.savez(d + f'/out{metric}.npz', ids=ids, sc=sc, cnt=cnt, evals=st.rows_scanned)\n"
    )
    env = dict(os.environ, NMN_HNSW_HOST_SEARCH="1")
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    for metric in METRICS:
        o = oracle(name, "high_speed", metric)
        out = np.load(tmp_path / f"out{metric}.npz")
        want, evals = want_answers(o, Q, 10, 0)
        assert_same((out["ids"], out["sc"], out["cnt"]), want)
        assert int(out["evals"]) == evals


# ---- memory and surface -----------------------------------------------------------------------------------------------------------------
def test_hbm_bytes_less_than_half_of_dense():
    """By the layouts at 2000 x 256 with capacity_hint = n: codes 512 000 + records 32 000 + adjacency against rows 2 048 000 +
    their 8-bit mirror and magnitudes + the same adjacency — about 0.82 MB against 2.3 MB."""
    from neumann_amd import GpuHnsw, synth_rows
    n, d = 2000, 256
    rows = synth_rows(0x5EED0021, 0, n, d)
    with GpuHnsw(d, g_cfg("high_speed", ho.COSINE), capacity_hint=n, storage="quantized") as gq, \
            GpuHnsw(d, g_cfg("high_speed", ho.COSINE), capacity_hint=n, storage="dense") as gd:
        gq.insert(rows)
        gd.insert(rows)
        print(f"hbm_bytes at {n} x {d}: quantized {gq.hbm_bytes}, dense {gd.hbm_bytes}")
        assert gq.hbm_bytes >= n * d + n * 16
        assert 2 * gq.hbm_bytes < gd.hbm_bytes
        st = gq.memory_stats()
        assert st["total_nodes"] == n and st["quantized_count"] == n and st["dense_count"] == 0
        assert st["embedding_bytes"] == n * (16 + d)
        st = gd.memory_stats()
        assert st["dense_count"] == n and st["quantized_count"] == 0 and st["embedding_bytes"] == n * d * 4


def test_surface_and_refusals():
    from neumann_amd import ExtendedDistanceMetric, GpuHnsw, HNSWConfig, NeumannGpuError, _capi
    with pytest.raises(NeumannGpuError) as e:                                       # Auto is refused by the new entry
        GpuHnsw(8, storage="auto")
    assert e.value.status == _capi.ERR_CONFIGURATION
    with pytest.raises(NeumannGpuError) as e:                                       # ... and the old field keeps its refusal
        GpuHnsw(8, HNSWConfig(storage="quantized"))
    assert e.value.status == _capi.ERR_CONFIGURATION
    with GpuHnsw(8, HNSWConfig(storage="auto"), storage="quantized") as g:          # cfg.storage is not read by the new entry
        assert g.storage == "quantized" and g.vectors() is None and len(g) == 0
        ids, sc, cnt = g.search(np.ones((2, 8), F), 3)                              # empty index
        assert cnt.tolist() == [0, 0]
        g.insert(np.eye(8, dtype=F))
        assert g.vectors() is None and g.hbm_bytes > 0
        with pytest.raises(NeumannGpuError, match="quantized") as e:
            g.search_metric(np.ones(8, F), 3, ExtendedDistanceMetric.Cosine)
        assert e.value.status == _capi.ERR_CONFIGURATION
        with pytest.raises(NeumannGpuError) as e:
            g.quantized_row(8)
        assert e.value.status == _capi.ERR_NOT_FOUND
        codes, scale, mn = g.quantized_row(3)                                        # a unit vector: range 1, codes 0 / 255
        assert codes.tolist() == [0, 0, 0, 255, 0, 0, 0, 0] and scale == F(F(1.0) / F(255.0)) and mn == F(0.0)
    with GpuHnsw(4, HNSWConfig(max_nodes=3), storage="quantized") as g:             # the max_nodes rule
        g.insert(np.eye(4, dtype=F)[:3])
        with pytest.raises(NeumannGpuError, match=r"HNSW index at capacity: 3 nodes \(limit: 3\)") as e:
            g.insert(np.ones((1, 4), F))
        assert e.value.status == _capi.ERR_CAPACITY and len(g) == 3


@pytest.mark.parametrize("metric", METRICS)
def test_dense_through_the_new_entry_builds_the_dense_graph(metric):
    from neumann_amd import GpuHnsw, NeumannGpuError, _capi
    name = "plain:360:20"
    rows, Q = corpus(name)
    o = ho.build(rows, o_cfg("high_speed", metric))
    with GpuHnsw(20, g_cfg("high_speed", metric), storage="dense") as g:
        g.insert(rows)
        assert g.storage == "dense" and g.vectors().rows == 360
        assert_graph(g, o)
        assert_same(g.search(Q, 10), ho.padded_answers(o, Q, 10))
        assert g.get_vector(7).tobytes() == rows[7].tobytes()
        with pytest.raises(NeumannGpuError) as e:
            g.quantized_row(0)
        assert e.value.status == _capi.ERR_CONFIGURATION
