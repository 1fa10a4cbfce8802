"""nmn_hnsw_* (neumann_amd.GpuHnsw) against tests/_hnsw_oracle.py: the graph nmn_hnsw_insert builds and every answer of
nmn_hnsw_search / nmn_hnsw_search_device — ids exact, score BITS equal, every query of every corpus compared in full."""
import functools
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

from tests import _hnsw_oracle as ho

pytestmark = pytest.mark.gpu
F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "hnsw_small.npz")
METRICS = [ho.COSINE, ho.EUCLIDEAN, ho.DOT_PRODUCT]
PRESETS = ["default", "high_recall", "high_speed"]


def o_cfg(preset, metric):
    c = {"default": ho.HNSWConfig, "high_recall": ho.HNSWConfig.high_recall, "high_speed": ho.HNSWConfig.high_speed}[preset]()
    return c.with_distance_metric(metric)


def g_cfg(preset, metric, **kw):
    from neumann_amd import HNSWConfig
    c = getattr(HNSWConfig, preset)().with_distance_metric(metric)
    for k, v in kw.items():
        setattr(c, k, v)
    return c


@functools.lru_cache(maxsize=None)
def corpus(name):
    """name -> (rows, queries)"""
    rng = np.random.default_rng(sum(map(ord, name)))
    kind, n, d = name.split(":")
    n, d = int(n), int(d)
    rows = (rng.standard_normal((n, d)) + 2.0 * rng.standard_normal((6, d))[rng.integers(0, 6, n)]).astype(F)
    if kind == "dup":      # a quarter of the rows are exact duplicates of earlier ones
        for i in range(4, n, 4):
            rows[i] = rows[rng.integers(0, i)]
    elif kind == "same":   # identical rows only
        rows[:] = rows[0]
    elif kind == "zeros":  # some zero rows (the distance 1.0 rule under Cosine)
        rows[::7] = 0.0
    queries = rng.standard_normal((40, d)).astype(F)
    queries[:10] = rows[rng.integers(0, n, 10)]
    if kind == "zeros":
        queries[10] = 0.0
    return rows, queries


@functools.lru_cache(maxsize=None)
def oracle(name, preset, metric):
    return ho.build(corpus(name)[0], o_cfg(preset, metric))


def gpu_index(name, preset, metric, batches=None, **cfg_kw):
    from neumann_amd import GpuHnsw
    rows = corpus(name)[0]
    g = GpuHnsw(rows.shape[1], g_cfg(preset, metric, **cfg_kw))
    if batches is None:
        ids = g.insert(rows)
        assert ids.tolist() == list(range(len(rows)))
    else:
        at = 0
        for b in batches:
            got = g.insert(rows[at:at + b])
            assert got.tolist() == list(range(at, min(at + b, len(rows))))
            at += b
        assert at >= len(rows)
    return g


def assert_graph(g, o):
    assert len(g) == len(o)
    assert g.entry_point == o.entry_point and g.max_layer == o.max_layer
    assert g.levels().tolist() == o.levels
    for node in range(len(o)):
        for layer in range(o.levels[node] + 1):
            assert g.neighbors(node, layer).tolist() == o.neighbors[node][layer], (node, layer)
        assert g.neighbors(node, o.levels[node] + 1).size == 0


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


# ---- the graph --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("preset", PRESETS)
@pytest.mark.parametrize("metric", METRICS)
def test_graph_equals_oracle(metric, preset):
    name = "plain:360:20"
    o = oracle(name, preset, metric)
    with gpu_index(name, preset, metric) as g:
        assert_graph(g, o)
    with gpu_index(name, preset, metric, batches=[1, 1, 7, 100, 3, 248]) as g:   # ragged batches: the same graph
        assert_graph(g, o)


@pytest.mark.parametrize("metric", METRICS)
def test_graph_and_answers_with_duplicates(metric):
    """ties: a quarter of the rows duplicate others; and a corpus of identical rows only"""
    for name in ("dup:400:16", "same:150:9"):
        o = oracle(name, "default", metric)
        Q = corpus(name)[1]
        with gpu_index(name, "default", metric) as g:
            assert_graph(g, o)
            for k, ef in ((1, None), (10, None), (50, None), (80, None), (10, 100), (400, None)):
                assert_same(g.search(Q, k, ef), ho.padded_answers(o, Q, k, ef))


# ---- search -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("preset", PRESETS)
@pytest.mark.parametrize("metric", METRICS)
def test_search_equals_oracle(metric, preset):
    name = "plain:360:20"
    o = oracle(name, preset, metric)
    Q = corpus(name)[1]
    efs = o.config.ef_search
    with gpu_index(name, preset, metric) as g:
        assert_same(g.search(Q[0], 5), ho.padded_answers(o, Q[0], 5))                     # nq = 1
        for k, ef in ((3, None), (efs, None), (efs + 30, None), (1000, None), (7, 11), (7, 300)):  # k < ef, = ef, > ef, > n, ef override
            ids, sc, cnt, st = g.search(Q, k, ef, with_stats=True)
            assert_same((ids, sc, cnt), ho.padded_answers(o, Q, k, ef))
            assert st.sweep == "graph" and st.rows_scanned > 0 and st.fallback_queries == 0
        big = np.concatenate([Q] * 8)[:300] + F(0.125) * np.arange(300, dtype=F)[:, None] / 300  # a batch of a few hundred
        assert_same(g.search(big, 10), ho.padded_answers(o, big, 10))


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("dim", [1, 3, 6, 8, 13, 33, 130])
def test_dimensions_and_tiny_indexes(dim, metric):
    """dims that are not multiples of 8 (scalar tail) or of 4 (row and query alignment); indexes of 0, 1 and 2 nodes"""
    from neumann_amd import GpuHnsw
    name = f"plain:90:{dim}"
    rows, Q = corpus(name)
    o = ho.HNSWIndex(o_cfg("default", metric))
    with GpuHnsw(dim, g_cfg("default", metric)) as g:
        ids, sc, cnt = g.search(Q, 4)                                                     # empty index
        assert cnt.tolist() == [0] * len(Q) and np.all(ids == np.uint64(0xFFFFFFFFFFFFFFFF)) and np.all(np.isneginf(sc))
        assert g.entry_point is None
        for upto in (1, 2, 90):
            while len(o) < upto:
                o.insert(rows[len(o)])
                g.insert(rows[len(o) - 1])
            assert_graph(g, o)
            assert_same(g.search(Q, 4), ho.padded_answers(o, Q, 4))                       # a search after a later insert sees the new nodes


@pytest.mark.parametrize("metric", METRICS)
def test_zero_rows_and_zero_query(metric):
    name = "zeros:200:12"
    o = oracle(name, "high_speed", metric)
    Q = corpus(name)[1]
    with gpu_index(name, "high_speed", metric) as g:
        assert_graph(g, o)
        assert_same(g.search(Q, 25), ho.padded_answers(o, Q, 25))
    if metric == ho.COSINE:  # a zero query is at distance 1.0 of everything: similarity 0.0
        _, sc, cnt = ho.padded_answers(o, Q[10], 5)
        assert cnt[0] == 5 and np.all(sc[0] == 0.0)


@pytest.mark.parametrize("metric", METRICS)
def test_overflow_paths(metric):
    """Reached by configuration: (a) ef above the 1024 results a wave keeps in LDS — every query goes to the spill launch;
    (b) the LDS candidate heap set to 8 entries (nmn_hnsw_set_heap_capacity), which the walks of this corpus exceed; (c) a results
    heap of 16 entries with ef_search 50.  All three return the oracle's answer."""
    name = "plain:1300:10"
    o = oracle(name, "high_speed", metric)
    Q = corpus(name)[1]
    with gpu_index(name, "high_speed", metric) as g:
        ids, sc, cnt, st = g.search(Q, 10, 1100, with_stats=True)                          # (a)
        assert_same((ids, sc, cnt), ho.padded_answers(o, Q, 10, 1100))
        assert st.fallback_queries == len(Q)
        want = ho.padded_answers(o, Q, 10, 50)
        g.set_heap_capacity(candidates=8)                                                  # (b)
        ids, sc, cnt, st = g.search(Q, 10, 50, with_stats=True)
        assert_same((ids, sc, cnt), want)
        assert st.fallback_queries > 0
        import torch
        got = g.search_device(dev(Q), 10, 50)                                              # ... stream-ordered too
        torch.cuda.synchronize()
        assert_same(host(got), want)
        g.set_heap_capacity(results=16)                                                    # (c)
        ids, sc, cnt, st = g.search(Q, 10, 50, with_stats=True)
        assert_same((ids, sc, cnt), want)
        assert st.fallback_queries == len(Q)
        g.set_heap_capacity()
        ids, sc, cnt, st = g.search(Q, 10, 50, with_stats=True)
        assert_same((ids, sc, cnt), want)
        assert st.fallback_queries == 0


def test_search_device_equals_search_and_pipelines():
    import torch
    name = "dup:400:16"
    for metric in METRICS:
        o = oracle(name, "default", metric)
        Q = corpus(name)[1]
        with gpu_index(name, "default", metric) as g:
            want = ho.padded_answers(o, Q, 10)
            got = g.search_device(dev(Q), 10)
            torch.cuda.synchronize()
            assert_same(host(got), want)
            assert_same(host(got), g.search(Q, 10))
            # pipelined calls on one stream, different shapes, outputs kept apart
            s = torch.cuda.Stream()
            qd = dev(Q)
            with torch.cuda.stream(s):
                outs = [g.search_device(qd[:n], k, ef, stream=s) for n, k, ef in ((40, 10, None), (1, 3, None), (17, 60, None), (40, 10, 120))]
            s.synchronize()
            for (n, k, ef), out in zip(((40, 10, None), (1, 3, None), (17, 60, None), (40, 10, 120)), outs):
                assert_same(host(out), ho.padded_answers(o, Q[:n], k, ef))
            # an insert waits for what is in flight and later searches see the new nodes
            with torch.cuda.stream(s):
                before = g.search_device(qd, 10, stream=s)
            extra = corpus("plain:90:16")[0][:30]
            g.insert(extra)
            s.synchronize()
            assert_same(host(before), want)
            o2 = ho.build(np.concatenate([corpus(name)[0], extra]), o_cfg("default", metric))
            after = g.search_device(qd, 10)
            torch.cuda.synchronize()
            assert_same(host(after), ho.padded_answers(o2, Q, 10))


def test_validation_and_refusals():
    from neumann_amd import GpuHnsw, HNSWConfig, NeumannGpuError, _capi
    with GpuHnsw(8) as g:
        g.insert(np.eye(8, dtype=F))
        with pytest.raises(NeumannGpuError) as e:
            g.search(np.ones(8, F), 0)
        assert e.value.status == _capi.ERR_INVALID_TOP_K
        ids, sc, cnt = g.search(np.zeros((0, 8), F), 3)                                   # nq = 0: nothing enqueued
        assert ids.shape == (0, 3)
        with pytest.raises(NeumannGpuError) as e:
            g.insert(np.ones((1, 7), F))
        assert e.value.status == _capi.ERR_DIMENSION_MISMATCH
        v = g.vectors()
        assert v.rows == 8 and v.dim == 8
        assert g.hbm_bytes > 8 * 8 * 4
    for storage in ("auto", "quantized"):
        with pytest.raises(NeumannGpuError) as e:
            GpuHnsw(8, HNSWConfig(storage=storage))
        assert e.value.status == _capi.ERR_CONFIGURATION
    with GpuHnsw(4, HNSWConfig(max_nodes=3)) as g:                                        # hnsw.rs:102-107, 1947-1955
        g.insert(np.eye(4, dtype=F)[:3])
        with pytest.raises(NeumannGpuError, match=r"HNSW index at capacity: 3 nodes \(limit: 3\)") as e:
            g.insert(np.ones((1, 4), F))
        assert e.value.status == _capi.ERR_CAPACITY and len(g) == 3


def test_exhaustive_search_over_the_same_rows():
    """nmn_hnsw_vectors hands the flat index out, node id == row: the exhaustive search finds a query that IS row i at row i"""
    from neumann_amd import DistanceMetric
    name = "plain:360:20"
    R, Q = corpus(name)
    with gpu_index(name, "default", ho.EUCLIDEAN) as g:
        v = g.vectors()
        assert v.rows == 360 and v.dim == 20
        rows, scores, counts = v.search(Q[:10], 1, DistanceMetric.Euclidean)
        for i in range(10):
            assert np.array_equal(R[int(rows[i, 0])], Q[i]) and scores[i, 0] == 1.0


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
        "    with GpuHnsw(rows.shape[1], HNSWConfig().with_distance_metric(metric)) as g:\n"
        "        g.insert(rows)\n"
        "        ids, sc, cnt, st = g.search(Q, 10, with_stats=True)\n"
        "        assert st.sweep_launches == 0, st.sweep_launches\n"
        "        np.savez(d + f'/out{metric}.npz', ids=ids, sc=sc, cnt=cnt)\n"
    )
    env = dict(os.environ, NMN_HNSW_HOST_SEARCH="1")
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    for metric in METRICS:
        o = oracle(name, "default", metric)
        out = np.load(tmp_path / f"out{metric}.npz")
        assert_same((out["ids"], out["sc"], out["cnt"]), ho.padded_answers(o, Q, 10))
        with gpu_index(name, "default", metric) as g:
            assert_same(g.search(Q, 10), (out["ids"], out["sc"], out["cnt"]))


def test_golden_file():
    from neumann_amd import GpuHnsw, HNSWConfig
    z = np.load(GOLDEN)
    m, m0, efc, efs, metric = z["config"].tolist()
    with GpuHnsw(z["rows"].shape[1], HNSWConfig(m=m, m0=m0, ef_construction=efc, ef_search=efs, distance_metric=metric)) as g:
        g.insert(z["rows"])
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


def test_concurrent_host_callers():
    name = "dup:400:16"
    o = oracle(name, "default", ho.COSINE)
    Q = corpus(name)[1]
    with gpu_index(name, "default", ho.COSINE) as g:
        alone = [g.search(Q[i:i + 5], 10) for i in range(0, 40, 5)]
        for a, i in zip(alone, range(0, 40, 5)):
            assert_same(a, ho.padded_answers(o, Q[i:i + 5], 10))
        got = [None] * 8
        errs = []

        def work(t):
            try:
                for _ in range(10):
                    got[t] = g.search(Q[5 * t:5 * t + 5], 10)
            except Exception as e:  # noqa: BLE001
                errs.append(e)

        th = [threading.Thread(target=work, args=(t,)) for t in range(8)]
        [t.start() for t in th]
        [t.join() for t in th]
        assert not errs, errs
        for a, b in zip(alone, got):
            assert_same(b, a)


def test_large_graph_gpu_walk_equals_host_walk():
    """CONSISTENCY, not parity: 30 000 nodes are beyond the Python oracle, so the GPU walk is compared with the library's own host
    walk (NMN_HNSW_HOST_SEARCH=1 is read at every call) — the code whose graph and answers the tests above hold to the oracle."""
    from neumann_amd import GpuHnsw, synth_rows
    n, d = 30000, 32
    rows = synth_rows(0x5EED0011, 0, n, d)
    Q = synth_rows(0x5EED0012, 0, 200, d)
    with GpuHnsw(d, g_cfg("high_speed", ho.EUCLIDEAN), capacity_hint=n) as g:
        g.insert(rows[:20000])
        g.insert(rows[20000:])
        assert len(g) == n
        gpu = [g.search(Q, 10), g.search(Q, 100, 150)]
        os.environ["NMN_HNSW_HOST_SEARCH"] = "1"
        try:
            cpu = [g.search(Q, 10), g.search(Q, 100, 150)]
        finally:
            del os.environ["NMN_HNSW_HOST_SEARCH"]
        for a, b in zip(gpu, cpu):
            assert_same(a, b)
        # and the walk is worth something: recall@10 against the exhaustive search over the same rows
        from neumann_amd import DistanceMetric
        ex_rows, _, _ = g.vectors().search(Q, 10, DistanceMetric.Euclidean)
        recall = np.mean([len(set(a.tolist()) & set(b.tolist())) / 10 for a, b in zip(gpu[1][0][:, :10], ex_rows)])
        print(f"recall@10 at ef 150, 30000 x 32, high_speed: {recall:.3f}")  # reported, not asserted: the graph is the algorithm's
