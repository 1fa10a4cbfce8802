"""EmbeddingStorage::Binary on the GPU (nmn_hnsw_create_binary, GpuHnsw(..., storage="binary")) against
tests/_hnsw_bin_oracle.py: every word and +-1 bit of every row, the graph nmn_hnsw_insert builds, and every answer of
nmn_hnsw_search / _search_multi / _search_device — ids exact, score BITS equal, every query compared in full."""
import ctypes as C
import functools
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

from tests import _hnsw_bin_oracle as hb
from tests import _hnsw_oracle as ho
from tests import _ivf_codec_oracle as co

pytestmark = pytest.mark.gpu
F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "hnsw_bin_small.npz")
METRICS = [ho.COSINE, ho.EUCLIDEAN, ho.DOT_PRODUCT]
THRESHOLDS = ["sign", "mean", "median"]
# 1: two codes, everything tied.  5: 32 codes, a tail only.  8: one chunk.  13: a chunk and a tail.  63 / 64 / 65: the word seam.
# 128: one 16-byte load, no remainder.  129: a full load, then a load that holds one tail bit.  200: an odd word count (4th word is
# padding), nine remaining chunks.  771: six full loads — more than the prefetch depth of four — then a chunk and a tail of three.
DIMS = [1, 5, 8, 13, 63, 64, 65, 128, 129, 200, 771]
N_ROWS = {1: 300, 5: 600, 771: 300}                        # every other dimension: 400


def o_cfg(metric):
    return ho.HNSWConfig.high_speed().with_distance_metric(metric)


def g_cfg(metric):
    from neumann_amd import HNSWConfig
    return HNSWConfig.high_speed().with_distance_metric(metric)


@functools.lru_cache(maxsize=None)
def corpus(name):
    """name = kind:n:dim -> (rows, queries): clustered normal rows; `dup`: a quarter exact duplicates; `same`: identical rows"""
    rng = np.random.default_rng(sum(map(ord, name)))
    kind, n, d = name.split(":")
    n, d = int(n), int(d)
    rows = (rng.standard_normal((n, d)) + 1.5 * rng.standard_normal((6, d))[rng.integers(0, 6, n)]).astype(F)
    if kind == "dup":
        for i in range(4, n, 4):
            rows[i] = rows[rng.integers(0, i)]
    elif kind == "same":
        rows[:] = rows[0]
    queries = rng.standard_normal((32, d)).astype(F)
    queries[:8] = rows[rng.integers(0, n, 8)]
    queries[8] = 0.0                                        # the zero query: Cosine distance 1.0 to every row
    for r in (rows, queries):
        r.setflags(write=False)
    return rows, queries


@functools.lru_cache(maxsize=None)
def oracle(name, metric, threshold):
    return hb.build(corpus(name)[0], o_cfg(metric), threshold)


def gpu_index(name, metric, threshold, batches=None, **kw):
    from neumann_amd import GpuHnsw
    rows = corpus(name)[0]
    g = GpuHnsw(rows.shape[1], g_cfg(metric), storage="binary", binary_threshold=threshold, **kw)
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
    """every word and every +-1 get_vector bit of every row"""
    for node in range(len(o)):
        assert np.array_equal(g.binary_row(node), o.words[node]), node
        assert g.get_vector(node).tobytes() == o.rows[node].tobytes() == o.get_vector(node).tobytes(), node


def assert_same(got, want):
    ig, sg, cg = got[:3]
    iw, sw, cw = want
    assert np.array_equal(cg, cw), (cg, cw)
    assert np.array_equal(ig, iw), np.argwhere(ig != iw)[:5]
    assert np.array_equal(np.ascontiguousarray(sg).view(np.uint32), np.ascontiguousarray(sw).view(np.uint32))


def dev(Q):
    import torch
    return torch.from_numpy(np.array(np.atleast_2d(Q), dtype=F)).cuda()                 # (a copy: the corpus arrays are read-only)


def host(res):
    ids, sc, counts = res
    return ids.cpu().numpy().view(np.uint64), sc.cpu().numpy(), counts.cpu().numpy().astype(np.uint32)


def want_answers(o, Q, k, ef):
    """(ids, scores, counts), evaluations the oracle made"""
    o.distance_evals = 0
    res = ho.padded_answers(o, Q, k, ef or None)
    return res, o.distance_evals


def want_multi(o, Q, ks, efs, kstride):
    ids = np.full((len(Q), kstride), np.uint64(0xFFFFFFFFFFFFFFFF), dtype=np.uint64)
    sc = np.full((len(Q), kstride), -np.inf, dtype=F)
    cnt = np.zeros(len(Q), dtype=np.uint32)
    o.distance_evals = 0
    for i, q in enumerate(Q):
        a, b, c = ho.padded_answers(o, q, int(ks[i]), int(efs[i]) or None)
        ids[i, :ks[i]], sc[i, :ks[i]], cnt[i] = a[0], b[0], c[0]
    return (ids, sc, cnt), o.distance_evals


def check_searches(g, o, Q, searches, device=True, multi=True):
    import torch
    for k, ef in searches:
        want, evals = want_answers(o, Q, k, ef)
        ids, sc, cnt, st = g.search(Q, k, ef or None, with_stats=True)
        assert_same((ids, sc, cnt), want)
        assert st.sweep == "graph" and st.rows_scanned == evals, (k, ef, st.rows_scanned, evals)
        assert st.bytes_scanned == evals * 8 * ((g.dim + 63) // 64)
        if device:
            got = g.search_device(dev(Q), k, ef or None)
            torch.cuda.synchronize()
            assert_same(host(got), want)
    if multi:                                               # a k and an ef per query, one launch
        ks = np.array([1, 3, 10, 25][:4] * (len(Q) // 4 + 1), dtype=np.uint32)[:len(Q)]
        efs = np.array([0, 7, 50, 10, 120][:5] * (len(Q) // 5 + 1), dtype=np.uint32)[:len(Q)]
        want, evals = want_multi(o, Q, ks, efs, 25)
        ids, sc, cnt, st = g.search_multi(Q, ks, efs, kstride=25, with_stats=True)
        assert_same((ids, sc, cnt), want)
        assert st.rows_scanned == evals


# ---- every dimension at which the kernel takes another path ---------------------------------------------------------------------------
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("dim", DIMS)
def test_dimensions(dim, metric):
    n = N_ROWS.get(dim, 400)
    threshold = THRESHOLDS[(DIMS.index(dim) + metric) % 3]
    name = f"plain:{n}:{dim}"
    o = oracle(name, metric, threshold)
    Q = corpus(name)[1]
    with gpu_index(name, metric, threshold) as g:
        assert g.storage == "binary" and g.binary_threshold == threshold and g.vectors() is None
        assert_graph(g, o)
        assert_rows(g, o)
        check_searches(g, o, Q, ((10, 50), (n + 5, 0)))
    if dim in (1, 5):                                       # at most 2 and 32 distinct codes: every distance is tied with many others
        assert len({w.tobytes() for w in o.words[:o.n]}) <= 2 ** dim


# ---- three metrics x three thresholds, and an insert in two batches against one ----------------------------------------------------------
@pytest.mark.parametrize("threshold", THRESHOLDS)
@pytest.mark.parametrize("metric", METRICS)
def test_metrics_and_thresholds(metric, threshold):
    name = "plain:360:20"
    o = oracle(name, metric, threshold)
    rows, Q = corpus(name)
    assert np.array_equal(o.words[:o.n], co.from_dense_rows(rows, threshold))
    with gpu_index(name, metric, threshold) as g:
        assert_graph(g, o)
        assert_rows(g, o)
        check_searches(g, o, Q, ((1, 0), (10, 50), (25, 10)))
    with gpu_index(name, metric, threshold, batches=[123, 237]) as g:
        assert_graph(g, o)
        assert_rows(g, o)
        check_searches(g, o, Q, ((10, 50),), device=False, multi=False)


# ---- identical rows, duplicated rows, the zero query --------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("name", ["dup:400:24", "same:150:9"])
def test_corpora(name, metric):
    threshold = "median" if name.startswith("dup") else "sign"
    o = oracle(name, metric, threshold)
    rows, Q = corpus(name)
    with gpu_index(name, metric, threshold) as g:
        assert_graph(g, o)
        assert_rows(g, o)
        check_searches(g, o, Q, ((10, 50), (len(rows) + 5, 0)))
        if metric == ho.COSINE:                             # the zero query: distance 1.0, similarity 0.0, in the walk's own order
            ids, sc, cnt = g.search(Q[8], 5)
            assert cnt[0] == 5 and np.all(sc[0] == 0.0)
            assert_same((ids, sc, cnt), want_answers(o, Q[8], 5, 0)[0])


def test_empty_and_one_node():
    import torch
    from neumann_amd import GpuHnsw
    with GpuHnsw(13, g_cfg(ho.COSINE), storage="binary", binary_threshold="mean") as g:
        assert len(g) == 0 and g.entry_point is None and g.hbm_bytes > 0
        ids, sc, cnt, st = g.search(np.ones((3, 13), F), 4, with_stats=True)
        assert cnt.tolist() == [0, 0, 0] and np.all(ids == np.uint64(0xFFFFFFFFFFFFFFFF)) and np.all(np.isneginf(sc))
        assert st.rows_scanned == 0 and st.sweep == "none"
        got = g.search_device(dev(np.ones((3, 13), F)), 4)
        torch.cuda.synchronize()
        assert host(got)[2].tolist() == [0, 0, 0]
        row = np.arange(13, dtype=F)
        g.insert(row)
        o = hb.build(row[None, :], o_cfg(ho.COSINE), "mean")
        assert_graph(g, o)
        assert_rows(g, o)
        Q = np.stack([row, -row, np.zeros(13, F)])
        assert_same(g.search(Q, 3), ho.padded_answers(o, Q, 3))
        assert_same(g.search_multi(Q, [1, 2, 3]), want_multi(o, Q, [1, 2, 3], [0, 0, 0], 3)[0])


def test_growth_past_the_first_allocation():
    """1100 x 8 in batches of 1000 and 100 with no capacity hint: the second batch outgrows the 1024 rows the word array was
    allocated for, so the words already inserted are sent again from the host's copy"""
    name = "plain:1100:8"
    o = oracle(name, ho.EUCLIDEAN, "mean")
    Q = corpus(name)[1]
    with gpu_index(name, ho.EUCLIDEAN, "mean", batches=[1000, 100]) as g:
        assert_graph(g, o)
        assert_rows(g, o)
        check_searches(g, o, Q, ((10, 50),))


# ---- both overflow paths ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", METRICS)
def test_lds_heap_overflow_goes_to_the_spill_launch(metric):
    import torch
    name = "plain:400:65"
    threshold = THRESHOLDS[(DIMS.index(65) + metric) % 3]  # (the oracle of test_dimensions)
    o = oracle(name, metric, threshold)
    Q = corpus(name)[1]
    want, evals = want_answers(o, Q, 10, 50)
    ks = np.array([1, 3, 10, 25] * 8, dtype=np.uint32)
    efs = np.array(([0, 7, 50, 10, 120] * 7)[:32], dtype=np.uint32)
    wantm, evalsm = want_multi(o, Q, ks, efs, 25)
    with gpu_index(name, metric, threshold) as g:
        g.set_heap_capacity(candidates=8)                   # the candidate heap fills up: flagged, answered by the spill launch
        ids, sc, cnt, st = g.search(Q, 10, 50, with_stats=True)
        assert_same((ids, sc, cnt), want)
        assert st.fallback_queries > 0 and st.rows_scanned == evals
        got = g.search_device(dev(Q), 10, 50)
        torch.cuda.synchronize()
        assert_same(host(got), want)
        ids, sc, cnt, st = g.search_multi(Q, ks, efs, kstride=25, with_stats=True)
        assert_same((ids, sc, cnt), wantm)
        assert st.fallback_queries > 0 and st.rows_scanned == evalsm
        g.set_heap_capacity(results=16)                     # the results heap does not fit: straight to the spill launch
        ids, sc, cnt, st = g.search(Q, 10, 50, with_stats=True)
        assert_same((ids, sc, cnt), want)
        assert st.fallback_queries == len(Q) and st.rows_scanned == evals
        ids, sc, cnt, st = g.search_multi(Q, ks, efs, kstride=25, with_stats=True)
        assert_same((ids, sc, cnt), wantm)
        assert st.fallback_queries > 0
        g.set_heap_capacity()
        ids, sc, cnt, st = g.search(Q, 10, 50, with_stats=True)
        assert_same((ids, sc, cnt), want)
        assert st.fallback_queries == 0


def test_host_search_env_in_child_process(tmp_path):
    """NMN_HNSW_HOST_SEARCH=1 (the walk on the host, the code insertion uses) in a fresh child process: the same bits"""
    name = "dup:400:24"
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
        "    with GpuHnsw(rows.shape[1], HNSWConfig.high_speed().with_distance_metric(metric), storage='binary',\n"
        "                 binary_threshold='median') as g:\n"
        "        g.insert(rows)\n"
        "        ids, sc, cnt, st = g.search(Q, 10, with_stats=True)\n"
        "        assert st.sweep_launches == 0, st.sweep_launches\n"
        "        np.savez(d + f'/out{metric}.npz', ids=ids, sc=sc, cnt=cnt, evals=st.rows_scanned)\n"
    )
    env = dict(os.environ, NMN_HNSW_HOST_SEARCH="1")
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    for metric in METRICS:
        o = oracle(name, metric, "median")
        out = np.load(tmp_path / f"out{metric}.npz")
        want, evals = want_answers(o, Q, 10, 0)
        assert_same((out["ids"], out["sc"], out["cnt"]), want)
        assert int(out["evals"]) == evals


# ---- eight threads through the coalescer ------------------------------------------------------------------------------------------------
def test_eight_threads_get_the_lone_call_bits():
    name = "plain:400:129"
    metric = ho.COSINE
    threshold = THRESHOLDS[(DIMS.index(129) + metric) % 3]
    o = oracle(name, metric, threshold)
    Q = corpus(name)[1]
    shapes = [(10, 50), (1, 0), (25, 10), (10, 50), (3, 120), (10, 0), (25, 10), (7, 7)]
    wants = [want_answers(o, Q[4 * t:4 * t + 4], k, ef) for t, (k, ef) in enumerate(shapes)]
    with gpu_index(name, metric, threshold) as g:
        lone = [g.search(Q[4 * t:4 * t + 4], k, ef or None) for t, (k, ef) in enumerate(shapes)]
        got, errs = [None] * 8, []
        start = threading.Barrier(8)

        def work(t):
            try:
                k, ef = shapes[t]
                start.wait()
                for _ in range(5):
                    got[t] = g.search(Q[4 * t:4 * t + 4], k, ef or None, with_stats=True)
                    assert_same(got[t], wants[t][0])
                    assert got[t][3].rows_scanned == wants[t][1]
            except BaseException as e:  # noqa: BLE001
                errs.append((t, repr(e)))

        threads = [threading.Thread(target=work, args=(t,)) for t in range(8)]
        for th in threads:
            th.start()
        for th in threads:
            th.join()
        assert not errs, errs
        for t in range(8):
            assert_same(got[t], lone[t])
            assert_same(lone[t], wants[t][0])
        batches, calls = g.coalesce_stats()                 # (batches that carried two or more calls, and the calls in them)
        assert 2 * batches <= calls


# ---- memory and surface -----------------------------------------------------------------------------------------------------------------
def test_memory_stats_and_hbm_bytes_below_a_quarter_of_dense():
    """By the layouts at 2000 x 256 with capacity_hint = n: words 2000 x 32 = 64 000 bytes + adjacency (about 0.27 MB) against the
    dense handle's rows, mirror, magnitudes and the same adjacency (about 2.9 MB, docs/hnsw.md §9).  A quarter leaves a factor of two."""
    from neumann_amd import GpuHnsw, synth_rows
    n, d = 2000, 256
    rows = synth_rows(0x5EED0021, 0, n, d)
    with GpuHnsw(d, g_cfg(ho.COSINE), capacity_hint=n, storage="binary") as gb, \
            GpuHnsw(d, g_cfg(ho.COSINE), capacity_hint=n, storage="dense") as gd:
        gb.insert(rows)
        gd.insert(rows)
        print(f"hbm_bytes at {n} x {d}: binary {gb.hbm_bytes}, dense {gd.hbm_bytes}")
        assert gb.binary_threshold == "sign" and gd.binary_threshold is None
        assert gb.hbm_bytes >= n * d // 8
        assert 4 * gb.hbm_bytes < gd.hbm_bytes
        st = gb.memory_stats()
        assert st["total_nodes"] == n and st["binary_count"] == n
        assert st["dense_count"] == st["quantized_count"] == st["sparse_count"] == 0
        assert st["embedding_bytes"] == n * 8 * (d // 64)
        assert gd.memory_stats()["binary_count"] == 0
    with GpuHnsw(65, g_cfg(ho.COSINE), storage="binary") as g:     # ceil(65 / 64) = 2 words
        g.insert(np.ones((3, 65), F))
        assert g.memory_stats()["embedding_bytes"] == 3 * 16
        assert g.binary_row(0).tolist() == [(1 << 64) - 1, 1]


def test_surface_and_refusals(tmp_path):
    """every entry a binary handle refuses: NMN_ERR_CONFIGURATION, a text that names the storage, nothing written, nothing inserted"""
    from neumann_amd import GpuHnsw, HNSWConfig, NeumannGpuError, _capi
    lib = _capi.load()
    with pytest.raises(NeumannGpuError) as e:               # the old field keeps refusing anything but dense
        GpuHnsw(8, HNSWConfig(storage="binary"))
    assert e.value.status == _capi.ERR_CONFIGURATION
    cfg = g_cfg(ho.COSINE)._c()
    cfg.storage = _capi.HNSW_STORAGE_BINARY
    h = C.c_void_p()
    assert lib.nmn_hnsw_create(C.byref(cfg), 8, 0, -1, C.byref(h)) == _capi.ERR_CONFIGURATION and not h
    cfg.storage = _capi.HNSW_STORAGE_DENSE
    assert lib.nmn_hnsw_create_binary(C.byref(cfg), 3, 8, 0, -1, C.byref(h)) == _capi.ERR_CONFIGURATION and not h
    with pytest.raises(NeumannGpuError):
        GpuHnsw(8, storage="binary", binary_threshold="mode")
    with pytest.raises(NeumannGpuError):
        GpuHnsw(8, storage="dense", binary_threshold="sign")
    # nmn_hnsw_create_with_storage(BINARY) is the Sign handle
    assert lib.nmn_hnsw_create_with_storage(C.byref(cfg), _capi.HNSW_STORAGE_BINARY, 8, 0, -1, C.byref(h)) == 0
    assert lib.nmn_hnsw_storage(h) == 3 and lib.nmn_hnsw_binary_threshold(h) == _capi.BINARY_SIGN
    lib.nmn_hnsw_destroy(h)

    with GpuHnsw(8, g_cfg(ho.COSINE), storage="binary", binary_threshold="mean") as g:
        g.insert(np.eye(8, dtype=F))
        assert g.storage == "binary" and g.binary_threshold == "mean" and g.vectors() is None
        assert g.binary_row(3).tolist() == [1 << 3]         # mean 1/8: only the one is above it
        with pytest.raises(NeumannGpuError) as e:
            g.binary_row(8)
        assert e.value.status == _capi.ERR_NOT_FOUND
        small = np.zeros(0, dtype=np.uint64)
        assert lib.nmn_hnsw_binary_row(g._h, 0, C.c_void_p(small.ctypes.data), 0) == _capi.ERR_BUFFER_TOO_SMALL

        SENT = 0x5A
        ids = np.full(64, SENT, dtype=np.uint8).view(np.uint64)
        sc = np.full(32, SENT, dtype=np.uint8).view(F)
        cnt = np.full(16, SENT, dtype=np.uint8).view(np.uint32)
        st = _capi.SearchStats()
        st.rows_scanned = 123
        q = np.ones((1, 8), F)
        one = np.ones(8, dtype=np.uint32)
        u64 = np.array([0, 1, 1], dtype=np.uint64)
        xm = _capi.XMetric(_capi.XMETRIC_COSINE, 0.0, 0.0, 0.0)
        p = lambda a: C.c_void_p(a.ctypes.data)              # noqa: E731
        path = str(tmp_path / "bin.hnsw").encode()
        calls = {
            "nmn_hnsw_search_metric": lambda: lib.nmn_hnsw_search_metric(g._h, p(q), 1, 2, C.byref(xm), p(ids), p(sc), p(cnt), C.byref(st)),
            "nmn_hnsw_search_metric_multi": lambda: lib.nmn_hnsw_search_metric_multi(g._h, p(q), 1, p(one), C.byref(xm), 2, p(ids), p(sc), p(cnt), C.byref(st)),
            "nmn_hnsw_search_metric_device": lambda: lib.nmn_hnsw_search_metric_device(g._h, p(q), 1, 2, C.byref(xm), p(ids), p(sc), p(cnt), None),
            "nmn_hnsw_search_sparse": lambda: lib.nmn_hnsw_search_sparse(g._h, p(u64), p(one), p(q), 1, 2, 0, p(ids), p(sc), p(cnt), C.byref(st)),
            "nmn_hnsw_search_sparse_multi": lambda: lib.nmn_hnsw_search_sparse_multi(g._h, p(u64), p(one), p(q), 1, p(one), None, 2, p(ids), p(sc), p(cnt), C.byref(st)),
            "nmn_hnsw_search_tt": lambda: lib.nmn_hnsw_search_tt(g._h, p(one), 1, p(one), p(u64), p(q), 1, 2, 0, p(ids), p(sc), p(cnt), C.byref(st)),
            "nmn_hnsw_search_tt_device": lambda: lib.nmn_hnsw_search_tt_device(g._h, p(one), 1, p(one), p(q), 1, 2, 0, p(ids), p(sc), p(cnt), None),
            "nmn_hnsw_cache_search": lambda: lib.nmn_hnsw_cache_search(g._h, p(q), 1, 2, 0.5, C.byref(xm), p(ids), p(sc), p(cnt), C.byref(st)),
            "nmn_hnsw_cache_search_sparse": lambda: lib.nmn_hnsw_cache_search_sparse(g._h, p(u64), p(one), p(q), 1, 2, 0.5, C.byref(xm), p(ids), p(sc), p(cnt), C.byref(st)),
            "nmn_hnsw_cache_search_device": lambda: lib.nmn_hnsw_cache_search_device(g._h, p(q), 1, 2, 0.5, C.byref(xm), p(ids), p(sc), p(cnt), None),
            "nmn_hnsw_set_node_mask": lambda: lib.nmn_hnsw_set_node_mask(g._h, p(u64), 1, 0),
            "nmn_hnsw_insert_sparse": lambda: lib.nmn_hnsw_insert_sparse(g._h, p(u64), p(one), p(q), 1, p(ids)),
            "nmn_hnsw_insert_auto": lambda: lib.nmn_hnsw_insert_auto(g._h, p(q), 1, p(ids)),
            "nmn_hnsw_insert_tt": lambda: lib.nmn_hnsw_insert_tt(g._h, p(one), 1, p(one), p(u64), p(q), 1, p(ids)),
            "nmn_hnsw_quantized_row": lambda: lib.nmn_hnsw_quantized_row(g._h, 0, p(ids), sc.ctypes.data_as(C.POINTER(C.c_float)), None),
            "nmn_hnsw_save": lambda: lib.nmn_hnsw_save(g._h, path),
        }
        for name, call in calls.items():
            assert call() == _capi.ERR_CONFIGURATION, name
            text = lib.nmn_last_error().decode()
            assert "Binary" in text, (name, text)
            assert np.all(ids.view(np.uint8) == SENT) and np.all(sc.view(np.uint8) == SENT) and np.all(cnt.view(np.uint8) == SENT), name
            assert st.rows_scanned == 123, name
            assert len(g) == 8 and g.node_live(0) == 1, name
        assert not os.path.exists(path)
        ids2, sc2, cnt2 = g.search(np.eye(8, dtype=F)[3], 1)                       # ... and the handle still answers
        assert cnt2[0] == 1 and ids2[0, 0] == 3
    with GpuHnsw(4, HNSWConfig(max_nodes=3), storage="binary") as g:              # the max_nodes rule
        g.insert(np.eye(4, dtype=F)[:3])
        with pytest.raises(NeumannGpuError, match=r"HNSW index at capacity: 3 nodes \(limit: 3\)") as e:
            g.insert(np.ones((1, 4), F))
        assert e.value.status == _capi.ERR_CAPACITY and len(g) == 3


# ---- the frozen golden file ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", hb.GOLDEN_METRICS)
@pytest.mark.parametrize("threshold", hb.GOLDEN_THRESHOLDS)
def test_golden_file(threshold, metric):
    from neumann_amd import GpuHnsw, HNSWConfig
    z = np.load(GOLDEN)
    p = f"{threshold}_{metric}_"
    with GpuHnsw(z["rows"].shape[1], HNSWConfig().with_distance_metric(metric), storage="binary", binary_threshold=threshold) as g:
        g.insert(z["rows"])
        for node in range(len(g)):
            assert np.array_equal(g.binary_row(node), z[f"words_{threshold}"][node])
        assert g.levels().tolist() == z[p + "levels"].tolist()
        assert g.entry_point == int(z[p + "entry_point"]) and g.max_layer == int(z[p + "max_layer"])
        for node in range(len(g)):
            c = int(z[p + "l0cnt"][node])
            assert g.neighbors(node, 0).tolist() == z[p + "l0"][node, :c].tolist()
        at = 0
        for node, layer, c in z[p + "up_head"].tolist():
            assert g.neighbors(node, layer).tolist() == z[p + "up_ids"][at:at + c].tolist()
            at += c
        assert_same(g.search(z["queries"], int(z["k"]), int(z["ef"])), (z[p + "ids"], z[p + "scores"], z[p + "counts"]))
