"""nmn_hnsw_insert_sparse / nmn_hnsw_insert_auto (GpuHnsw.insert_sparse / insert_auto / sparse_row) against
tests/_hnsw_mixed_oracle.py: a dense handle that holds Sparse and Dense nodes side by side — levels, every neighbour list, the entry
point, ids and score BITS, through every search entry (docs/hnsw.md §15)."""
import ctypes as C
import functools
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

from tests import _hnsw_mixed_oracle as mo
from tests import _hnsw_oracle as ho

pytestmark = pytest.mark.gpu
F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "hnsw_mixed_small.npz")
METRICS = [ho.COSINE, ho.EUCLIDEAN, ho.DOT_PRODUCT]
SV = mo.SparseVector
NONE64 = np.uint64(0xFFFFFFFFFFFFFFFF)


def o_cfg(metric, **kw):
    c = ho.HNSWConfig.high_speed().with_distance_metric(metric)
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def g_cfg(metric, **kw):
    from neumann_amd import HNSWConfig
    c = HNSWConfig.high_speed().with_distance_metric(metric)
    for k, v in kw.items():
        setattr(c, k, v)
    return c


@functools.lru_cache(maxsize=None)
def corpus(name):
    """name = kind:n:dim -> (rows, sparse mask, dense queries).  Clustered rows; a row inserted Sparse has 70 % zeros and is doubled
    (so that it reaches the answers under DotProduct).  inter: kinds interleaved, so every pass of a hop holds both; all: every row
    Sparse; special: also duplicates of earlier rows (of either kind) and all-zero rows of either kind."""
    rng = np.random.default_rng(sum(map(ord, name)))
    kind, n, d = name.split(":")
    n, d = int(n), int(d)
    rows = (rng.standard_normal((n, d)) + 2.0 * rng.standard_normal((6, d))[rng.integers(0, 6, n)]).astype(F)
    mask = np.ones(n, dtype=bool) if kind == "all" else np.arange(n) % 2 == 1
    rows[mask] = mo.sparsify(rng, rows[mask], 0.7) * F(2.0)
    if kind == "special":
        for i in range(5, n, 5):
            rows[i] = rows[rng.integers(0, i)]      # the row of another node, inserted with this node's kind
        rows[::37] = 0.0
        rows[1::41] = 0.0
    Q = rng.standard_normal((16, d)).astype(F)
    Q[8:][rng.random(Q[8:].shape) < 0.7] = 0.0
    Q[:3] = rows[rng.integers(0, n, 3)]
    return rows, mask, Q


@functools.lru_cache(maxsize=None)
def oracle(name, metric):
    rows, mask, _ = corpus(name)
    return mo.build_mixed(rows, mask, o_cfg(metric))


def insert_mixed(g, rows, mask):
    """runs of equal kind, each one call: insert for Dense rows, insert_sparse(from_dense) for Sparse ones"""
    i, n = 0, len(rows)
    while i < n:
        j = i
        while j < n and mask[j] == mask[i]:
            j += 1
        if mask[i]:
            g.insert_sparse(*g.sparse_from_dense(rows[i:j]))
        else:
            g.insert(rows[i:j])
        i = j


def gpu_index(name, metric):
    from neumann_amd import GpuHnsw
    rows, mask, _ = corpus(name)
    g = GpuHnsw(rows.shape[1], g_cfg(metric))
    insert_mixed(g, rows, mask)
    return g


def assert_graph(g, o):
    assert len(g) == len(o)
    assert g.entry_point == o.entry_point and g.max_layer == o.max_layer
    assert g.levels().tolist() == o.levels
    for node in range(len(o)):
        for layer in range(o.levels[node] + 1):
            assert g.neighbors(node, layer).tolist() == o.neighbors[node][layer], (node, layer)


def bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


def assert_same(got, want):
    ig, sg, cg = got[:3]
    iw, sw, cw = want[:3]
    assert np.array_equal(cg, cw), (cg, cw)
    assert np.array_equal(ig, iw), np.argwhere(ig != iw)[:5]
    assert np.array_equal(bits(sg), bits(sw)), np.argwhere(bits(sg) != bits(sw))[:5]


def dev(Q):
    import torch
    return torch.from_numpy(np.ascontiguousarray(np.atleast_2d(Q), dtype=F)).cuda()


def host(res):
    import torch
    torch.cuda.synchronize()
    ids, sc, counts = res
    return ids.cpu().numpy().view(np.uint64), sc.cpu().numpy(), counts.cpu().numpy().astype(np.uint32)


def expected_rows_scanned(o, nq, evals):
    """the dense handle's convention (docs/hnsw.md §9): the entry's distance is carried from layer to layer"""
    return evals if len(o) == 0 else evals - nq * o.max_layer


def every_entry(g, o, Q, k=10, ef=50):
    """dense queries Q and their from_dense() forms through all five search entries, held to the oracle"""
    dim = Q.shape[1]
    o.distance_evals = 0
    want_d = mo.answers_dense(o, Q, k, ef)
    evals_d = o.distance_evals
    sqs = [SV.from_dense(q) for q in Q]
    o.distance_evals = 0
    want_s = mo.answers_sparse(o, sqs, k, ef)
    evals_s = o.distance_evals
    ids, sc, cnt, st = g.search(Q, k, ef, with_stats=True)
    assert_same((ids, sc, cnt), want_d)
    assert st.sweep == "graph" and st.rows_scanned == expected_rows_scanned(o, len(Q), evals_d), (st.rows_scanned, evals_d)
    assert_same(host(g.search_device(dev(Q), k, ef)), want_d)
    csr = g.sparse_from_dense(Q)
    ids, sc, cnt, st = g.search_sparse(*csr, k, ef, with_stats=True)
    assert_same((ids, sc, cnt), want_s)
    assert st.rows_scanned == expected_rows_scanned(o, len(Q), evals_s), (st.rows_scanned, evals_s)
    # a k and an ef per query
    ks = np.array([1 + (3 * i) % 12 for i in range(len(Q))], dtype=np.uint32)
    efs = np.array([0, 20, 64, 7][: 4] * (len(Q) // 4 + 1), dtype=np.uint32)[: len(Q)]
    kmax = int(ks.max())
    gd = g.search_multi(Q, ks, efs)
    gs = g.search_sparse_multi(*csr, ks, efs)
    for i in range(len(Q)):
        e = o.config.ef_search if efs[i] == 0 else int(efs[i])
        wd = mo.padded([o.search_with_ef(Q[i], int(ks[i]), e)], kmax)
        ws = mo.padded([o.search_sparse_with_ef(sqs[i], int(ks[i]), e)], kmax)
        assert_same((gd[0][i:i + 1], gd[1][i:i + 1], gd[2][i:i + 1]), wd)
        assert_same((gs[0][i:i + 1], gs[1][i:i + 1], gs[2][i:i + 1]), ws)
    return want_d, want_s


# ---- 1. the golden corpus, and what a densifying shortcut would answer -------------------------------------------------------------
def golden_index(z, name, metric):
    idx = mo.HNSWMixedIndex(ho.HNSWConfig().with_distance_metric(metric))
    rows, mask = z["rows"], z["sparse_mask"]
    idx.n = len(rows)
    idx.levels = z[f"{name}_levels"].tolist()
    idx.entry_point, idx.max_layer = int(z[f"{name}_entry_point"]), int(z[f"{name}_max_layer"])
    idx.neighbors = [[[] for _ in range(lv + 1)] for lv in idx.levels]
    for node in range(idx.n):
        idx.neighbors[node][0] = z[f"{name}_l0"][node, : z[f"{name}_l0cnt"][node]].tolist()
    at = 0
    for node, layer, count in z[f"{name}_up_head"].tolist():
        idx.neighbors[node][layer] = z[f"{name}_up_ids"][at: at + count].tolist()
        at += count
    return idx


@pytest.mark.parametrize("name,metric,floor", [("dot", ho.DOT_PRODUCT, 32), ("cosine", ho.COSINE, 8)])
def test_golden_corpus(name, metric, floor):
    from neumann_amd import GpuHnsw, HNSWConfig
    z = np.load(GOLDEN)
    rows, mask, Q = z["rows"], z["sparse_mask"], z["queries"]
    with GpuHnsw(rows.shape[1], HNSWConfig().with_distance_metric(metric)) as g, \
            GpuHnsw(rows.shape[1], HNSWConfig().with_distance_metric(metric)) as twin:
        insert_mixed(g, rows, mask)
        assert_graph(g, golden_index(z, name, metric))
        got = g.search(Q, 10, 50)
        assert_same(got, (z[f"{name}_ids"], z[f"{name}_scores"], z[f"{name}_counts"]))
        assert_same(host(g.search_device(dev(Q), 10, 50)), got)
        assert_same(g.search_sparse(*g.sparse_from_dense(Q), 10, 50),
                    (z[f"{name}_sparse_ids"], z[f"{name}_sparse_scores"], z[f"{name}_sparse_counts"]))
        twin.insert(np.stack([g.get_vector(i) for i in range(len(rows))]))      # the all-dense handle over the to_dense() rows
        tw = twin.search(Q, 10, 50)
        assert_same(tw, (z[f"{name}_dense_ids"], z[f"{name}_dense_scores"], got[2]))
        differ = int(((got[0] != tw[0]) | (bits(got[1]) != bits(tw[1]))).any(axis=1).sum())
        print(f"{name}: {differ} of {len(Q)} answers differ from the all-dense handle")
        assert differ == int(z[f"{name}_differ"]) and differ >= floor
        assert g.hbm_bytes > twin.hbm_bytes


# ---- 2. metrics x dimensions, kinds interleaved; every entry -----------------------------------------------------------------------
@pytest.mark.parametrize("dim", [20, 33])
@pytest.mark.parametrize("metric", METRICS)
def test_metrics_interleaved_kinds(metric, dim):
    name = f"inter:200:{dim}"
    o = oracle(name, metric)
    with gpu_index(name, metric) as g:
        assert_graph(g, o)
        every_entry(g, o, corpus(name)[2])
        Q = corpus(name)[2]
        assert_same(g.search(Q, 205, None), mo.answers_dense(o, Q, 205, None))           # k > n: every node the walk reaches
        assert_same(g.search_sparse(*g.sparse_from_dense(Q), 205, None), mo.answers_sparse(o, [SV.from_dense(q) for q in Q], 205, None))


@pytest.mark.parametrize("dim,metric", [(5, ho.COSINE), (8, ho.DOT_PRODUCT), (128, ho.COSINE), (771, ho.DOT_PRODUCT)])
def test_dimensions(dim, metric):
    name = f"inter:120:{dim}"
    o = oracle(name, metric)
    with gpu_index(name, metric) as g:
        assert_graph(g, o)
        every_entry(g, o, corpus(name)[2][:8])


# ---- 3. entry counts around the pair split and the four-in-flight boundary; special rows; special queries ---------------------------
def counted_vectors(dim, rng):
    """Sparse nodes of 0, 1, 7, 8, 9 and dim entries, several of each, between Dense rows"""
    svs = []
    for rep in range(6):
        for nnz in (0, 1, 7, 8, 9, dim):
            pos = np.sort(rng.choice(dim, nnz, replace=False))
            svs.append(SV.from_parts(dim, pos.tolist(), (rng.standard_normal(nnz) * 2).astype(F)))
    return svs


def special_queries(dim, rows):
    full = rows[5].copy()
    full[full == 0] = F(-1.25)
    one = np.zeros(dim, dtype=F)
    one[dim - 1] = 2.5
    return np.stack([np.zeros(dim, dtype=F), one, full])      # entry-less, one entry, every position stored


@pytest.mark.parametrize("metric", METRICS)
def test_entry_counts_and_special_queries(metric):
    from neumann_amd import GpuHnsw
    dim = 20
    rng = np.random.default_rng(77)
    svs = counted_vectors(dim, rng)
    dense = rng.standard_normal((len(svs), dim)).astype(F)
    o = mo.HNSWMixedIndex(o_cfg(metric))
    with GpuHnsw(dim, g_cfg(metric)) as g:
        for s, d in zip(svs, dense):
            o.insert_sparse(s)
            o.insert(d)
            assert g.insert_sparse(*mo.csr_of([s])).tolist() == [len(o) - 2]
            assert g.insert(d).tolist() == [len(o) - 1]
        assert_graph(g, o)
        for node, s in enumerate(svs):
            p, v = g.sparse_row(2 * node)
            assert p.tolist() == s.positions and np.array_equal(bits(v), bits(s.values))
            assert g.sparse_row(2 * node + 1) is None
            assert np.array_equal(bits(g.get_vector(2 * node)), bits(s.to_dense()))
        Q = np.concatenate([special_queries(dim, dense), rng.standard_normal((5, dim)).astype(F)])
        want_d, want_s = every_entry(g, o, Q)
        if metric == ho.COSINE:
            assert np.all(want_d[1][0] == 0.0) and np.all(want_s[1][0] == 0.0)     # a zero query: every distance 1.0, the ties decide


@pytest.mark.parametrize("metric", METRICS)
def test_duplicate_and_zero_rows(metric):
    name = "special:185:12"
    o = oracle(name, metric)
    with gpu_index(name, metric) as g:
        assert_graph(g, o)
        every_entry(g, o, corpus(name)[2][:8])


@pytest.mark.parametrize("metric", [ho.COSINE, ho.DOT_PRODUCT])
def test_all_sparse_handle_and_one_node(metric):
    from neumann_amd import GpuHnsw
    name = "all:150:20"
    o = oracle(name, metric)
    with gpu_index(name, metric) as g:
        assert_graph(g, o)
        every_entry(g, o, corpus(name)[2][:8])
        ms = g.memory_stats()
        assert ms["sparse_count"] == 150 and ms["dense_count"] == 0
    s = SV.from_parts(6, [4, 1], [2.0, -3.0])
    one = mo.HNSWMixedIndex(o_cfg(metric))
    one.insert_sparse(s)
    with GpuHnsw(6, g_cfg(metric)) as g:
        g.insert_sparse([0, 2], [4, 1], [2.0, -3.0])
        assert_graph(g, one)
        every_entry(g, one, np.array([[0, 1, 0, 0, 1, 0], [1, 1, 1, 1, 1, 1]], dtype=F), k=3)


# ---- 4. insert_auto ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("threshold", [0.0, 0.5, 1.0])
def test_insert_auto(threshold):
    from neumann_amd import GpuHnsw
    rng = np.random.default_rng(int(threshold * 10) + 3)
    n, dim = 150, 16
    rows = rng.standard_normal((n, dim)).astype(F)
    share = rng.choice([0.0, 0.25, 0.5, 0.75, 1.0], n)
    for i in range(n):
        rows[i, rng.permutation(dim)[: int(share[i] * dim)]] = 0.0     # sparsity exactly 0, 0.25, 0.5 (the threshold itself), 0.75, 1
    rows[3, 2] = -0.0
    o = mo.HNSWMixedIndex(o_cfg(ho.COSINE, sparsity_threshold=threshold))
    for r in rows:
        o.insert_auto(r)
    with GpuHnsw(dim, g_cfg(ho.COSINE, sparsity_threshold=threshold)) as g:
        assert g.insert_auto(rows).tolist() == list(range(n))
        kinds = ["dense" if g.sparse_row(i) is None else "sparse" for i in range(n)]
        assert kinds == [o.kind(i) for i in range(n)]
        assert len(set(kinds)) == (1 if threshold == 0.0 else 2)
        assert_graph(g, o)
        for i in range(n):
            assert np.array_equal(bits(g.get_vector(i)), bits(o.rows[i]))
        ms = g.memory_stats()
        want = o.memory_stats()
        assert {k: ms[k] for k in want} == want
        every_entry(g, o, rng.standard_normal((6, dim)).astype(F))
    from neumann_amd import HNSWConfig
    with GpuHnsw(4, HNSWConfig(sparsity_threshold=float("nan"))) as g:      # a NaN threshold: Dense, whatever the row
        g.insert_auto(np.array([[0, 0, 0, 0], [np.nan, 0, 0, 0]], dtype=F))
        assert g.sparse_row(0) is None and g.sparse_row(1) is None
    with GpuHnsw(4, HNSWConfig(sparsity_threshold=0.75)) as g:              # a NaN element counts as stored: sparsity 0.75
        g.insert_auto(np.array([[np.nan, 0, 0, 0]], dtype=F))
        p, v = g.sparse_row(0)
        assert p.tolist() == [0] and np.isnan(v[0])


# ---- 5. search_metric is the walk with k = c plus the re-rank over the handle's rows ------------------------------------------------------
def test_search_metric_is_search_plus_rerank():
    from neumann_amd import ExtendedDistanceMetric as M
    name = "inter:200:20"
    Q = corpus(name)[2]
    with gpu_index(name, ho.COSINE) as g:
        for metric, top_k in ((M.Euclidean, 5), (M.Manhattan, 12)):
            c = max(2 * top_k, 10)
            ids, _, cnt = g.search(Q, c)
            want_ids = np.full((len(Q), top_k), NONE64, dtype=np.uint64)
            want_sc = np.full((len(Q), top_k), -np.inf, dtype=F)
            for i in range(len(Q)):
                cand = ids[i, : cnt[i]]
                sim = g.vectors().score_rows_xmetric(Q[i], cand, metric)[1][0]
                order = sorted(range(len(cand)), key=lambda t: -float(sim[t]))[:top_k]      # stable, descending
                want_ids[i, : len(order)] = cand[order]
                want_sc[i, : len(order)] = sim[order]
            got = g.search_metric(Q, top_k, metric)
            assert_same(got, (want_ids, want_sc, np.minimum(cnt, top_k).astype(np.uint32)))
            assert_same(host(g.search_metric_device(dev(Q), top_k, metric)), got)


# ---- 6. both overflow paths ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", [ho.COSINE, ho.DOT_PRODUCT])
def test_overflow_paths(metric):
    name = "inter:200:20"
    o = oracle(name, metric)
    Q = corpus(name)[2]
    want_d = mo.answers_dense(o, Q, 10, 50)
    want_s = mo.answers_sparse(o, [SV.from_dense(q) for q in Q], 10, 50)
    with gpu_index(name, metric) as g:
        csr = g.sparse_from_dense(Q)
        for kw, spilled in (({"results": 0, "candidates": 16}, None), ({"results": 16}, len(Q)), ({}, 0)):
            g.set_heap_capacity(**kw)
            ids, sc, cnt, st = g.search(Q, 10, 50, with_stats=True)
            assert_same((ids, sc, cnt), want_d)
            assert (st.fallback_queries > 0) if spilled is None else st.fallback_queries == spilled
            ids, sc, cnt, st = g.search_sparse(*csr, 10, 50, with_stats=True)
            assert_same((ids, sc, cnt), want_s)
            assert (st.fallback_queries > 0) if spilled is None else st.fallback_queries == spilled
            assert_same(host(g.search_device(dev(Q), 10, 50)), want_d)


# ---- 7. the host walk, in a fresh child process ---------------------------------------------------------------------------------------
def test_host_search_env_in_child_process(tmp_path):
    name = "inter:200:20"
    rows, mask, Q = corpus(name)
    np.savez(tmp_path / "in.npz", rows=rows, mask=mask, Q=Q)
    code = (
        "import sys, numpy as np\n"
        f"sys.path.insert(0, {ROOT!r})\n"
        "from neumann_amd import GpuHnsw, HNSWConfig\n"
        f"d = {str(tmp_path)!r}\n"
        "z = np.load(d + '/in.npz')\n"
        "rows, mask, Q = z['rows'], z['mask'], z['Q']\n"
        "for metric in (0, 1, 2):\n"
        "    with GpuHnsw(rows.shape[1], HNSWConfig.high_speed().with_distance_metric(metric)) as g:\n"
        "        for i in range(len(rows)):\n"
        "            g.insert_sparse(*g.sparse_from_dense(rows[i])) if mask[i] else g.insert(rows[i])\n"
        "        ids, sc, cnt, st = g.search(Q, 10, 50, with_stats=True)\n"
        "        assert st.sweep_launches == 0, st.sweep_launches\n"
        "        sids, ssc, scnt, st = g.search_sparse(*g.sparse_from_dense(Q), 10, 50, with_stats=True)\n"
        "        assert st.sweep_launches == 0, st.sweep_launches\n"
        "        np.savez(d + f'/out_{metric}.npz', ids=ids, sc=sc, cnt=cnt, sids=sids, ssc=ssc, scnt=scnt)\n"
    )
    env = dict(os.environ, NMN_HNSW_HOST_SEARCH="1")
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    sqs = [SV.from_dense(q) for q in Q]
    for metric in METRICS:
        o = oracle(name, metric)
        out = np.load(tmp_path / f"out_{metric}.npz")
        assert_same((out["ids"], out["sc"], out["cnt"]), mo.answers_dense(o, Q, 10, 50))
        assert_same((out["sids"], out["ssc"], out["scnt"]), mo.answers_sparse(o, sqs, 10, 50))


# ---- 8. what the device does not walk: the host answers, the same bits ------------------------------------------------------------------
@pytest.mark.parametrize("metric", [ho.COSINE, ho.DOT_PRODUCT])
def test_duplicated_positions_route_to_the_host(metric):
    name = "inter:200:20"
    rows, mask, Q = corpus(name)
    o = mo.build_mixed(rows, mask, o_cfg(metric))
    dupq = SV.from_parts(20, [3, 7, 3, 11, 7], [1.5, -2.0, 4.0, 0.5, 8.0])
    sqs = [SV.from_dense(q) for q in Q[:6]] + [dupq]
    csr = mo.csr_of(sqs)
    with gpu_index(name, metric) as g:
        # a query with a duplicated position, in a call with others that stay on the device
        ids, sc, cnt, st = g.search_sparse(*csr, 10, 50, with_stats=True)
        assert_same((ids, sc, cnt), mo.answers_sparse(o, sqs, 10, 50))
        # a NODE with a duplicated position: every sparse query of the handle is the host's from now on
        dup_node = SV.from_parts(20, [5, 2, 5, 19], [1.0, -1.0, 3.0, 2.0])
        o.insert_sparse(dup_node)
        g.insert_sparse(*mo.csr_of([dup_node]))
        assert_graph(g, o)
        p, v = g.sparse_row(len(o) - 1)
        assert p.tolist() == [2, 5, 5, 19] and v.tolist() == [-1.0, 1.0, 3.0, 2.0]
        assert g.get_vector(len(o) - 1)[5] == 3.0                                   # to_dense(): the last entry wins
        o.insert(rows[0])
        g.insert(rows[0])
        assert_graph(g, o)
        assert_same(g.search_sparse(*csr, 10, 50), mo.answers_sparse(o, sqs, 10, 50))
        ks = np.arange(1, len(sqs) + 1, dtype=np.uint32)
        got = g.search_sparse_multi(*csr, ks, None)
        for i, s in enumerate(sqs):
            assert_same((got[0][i:i + 1], got[1][i:i + 1], got[2][i:i + 1]), mo.padded([o.search_sparse_with_ef(s, int(ks[i]), 20)], len(sqs)))
        assert_same(g.search(Q, 10, 50), mo.answers_dense(o, Q, 10, 50))            # dense queries stay on the device
        assert_same(host(g.search_device(dev(Q), 10, 50)), mo.answers_dense(o, Q, 10, 50))


# (Euclidean with a sparse query — the union merge on the host — is part of test_metrics_interleaved_kinds and its siblings)


# ---- 9. refusals, with nothing inserted or written --------------------------------------------------------------------------------------
def test_refusals(tmp_path):
    from neumann_amd import GpuHnsw, NeumannGpuError, _capi
    with GpuHnsw(6, g_cfg(ho.COSINE), storage="quantized") as g:
        for call in (lambda: g.insert_sparse([0, 1], [0], [1.0]), lambda: g.insert_auto(np.zeros((1, 6), dtype=F))):
            with pytest.raises(NeumannGpuError) as e:
                call()
            assert e.value.status == _capi.ERR_CONFIGURATION and len(g) == 0
        g.insert(np.eye(6, dtype=F))
        assert g.sparse_row(0) is None
    with GpuHnsw(6, g_cfg(ho.COSINE, max_nodes=3)) as g:
        g.insert_sparse([0, 1, 2], [0, 1], [1.0, 1.0])
        with pytest.raises(NeumannGpuError) as e:
            g.insert_sparse([0, 1, 2, 3], [0, 6, 2], [1.0, 1.0, 1.0])              # a position == dim in the LAST row... of a batch
        assert e.value.status == _capi.ERR_INVALID_ARGUMENT and len(g) == 2          # ... that would also pass max_nodes
        assert "index 6" in str(e.value) and "dimension 6" in str(e.value)
        with pytest.raises(NeumannGpuError) as e:
            g.insert_sparse([0, 2, 1], [0, 1], [1.0, 1.0])
        assert e.value.status == _capi.ERR_INVALID_ARGUMENT and len(g) == 2
        for call in (lambda: g.insert_sparse([0, 1, 2], [0, 1], [1.0, 1.0]), lambda: g.insert_auto(np.ones((2, 6), dtype=F))):
            with pytest.raises(NeumannGpuError) as e:
                call()
            assert e.value.status == _capi.ERR_CAPACITY and len(g) == 2
            assert "HNSW index at capacity: 2 nodes (limit: 3)" in str(e.value)
        path = tmp_path / "mixed.idx"
        with pytest.raises(NeumannGpuError) as e:
            g.save(str(path))
        assert e.value.status == _capi.ERR_CONFIGURATION and "sparse" in str(e.value) and not path.exists()
        with pytest.raises(NeumannGpuError) as e:
            g.sparse_row(2)
        assert e.value.status == _capi.ERR_NOT_FOUND
        nnz = C.c_uint32(0)
        pos = np.zeros(1, dtype=np.uint32)
        st = g._lib.nmn_hnsw_sparse_row(g._h, 0, C.c_void_p(pos.ctypes.data), None, 0, C.byref(nnz))
        assert st == _capi.ERR_BUFFER_TOO_SMALL and nnz.value == 1


# ---- 10. a handle without sparse nodes is what it was ------------------------------------------------------------------------------------
def test_a_handle_without_sparse_nodes_answers_and_saves_as_before(tmp_path):
    from neumann_amd import GpuHnsw
    name = "inter:200:20"
    rows, _, Q = corpus(name)
    o = ho.build(rows, o_cfg(ho.COSINE))
    with GpuHnsw(20, g_cfg(ho.COSINE, sparsity_threshold=2.0)) as g, GpuHnsw(20, g_cfg(ho.COSINE, sparsity_threshold=2.0)) as plain:
        g.insert_auto(rows)                      # no sparsity reaches 2.0: insert_auto is insert
        plain.insert(rows)
        assert_graph(g, o)
        assert g.hbm_bytes == plain.hbm_bytes and g.memory_stats() == plain.memory_stats()
        assert g.memory_stats()["sparse_count"] == 0
        assert_same(g.search(Q, 10, 50), ho.padded_answers(o, Q, 10, 50))
        assert_same(g.search_sparse(*g.sparse_from_dense(Q), 10, 50), plain.search_sparse(*plain.sparse_from_dense(Q), 10, 50))
        g.save(str(tmp_path / "a.idx"))
        plain.save(str(tmp_path / "b.idx"))
        assert (tmp_path / "a.idx").read_bytes() == (tmp_path / "b.idx").read_bytes()


# ---- 11. concurrency: dense and sparse callers on a mixed handle ----------------------------------------------------------------------------
def test_dense_and_sparse_callers_on_a_mixed_handle():
    name = "inter:200:20"
    rows, mask, Q = corpus(name)
    o = oracle(name, ho.COSINE)
    with gpu_index(name, ho.COSINE) as g:
        csr = g.sparse_from_dense(Q)
        alone_sparse = g.search_sparse(*csr, 10, 50)
        alone_dense = g.search(Q, 10, 50)
        assert_same(alone_dense, mo.answers_dense(o, Q, 10, 50))
        assert_same(alone_sparse, mo.answers_sparse(o, [SV.from_dense(q) for q in Q], 10, 50))
        out, errs = [[] for _ in range(8)], []

        def run(t):
            try:
                for _ in range(12):
                    out[t].append(g.search_sparse(*csr, 10, 50) if t % 2 else g.search(Q, 10, 50))
            except Exception as e:  # noqa: BLE001
                errs.append(e)

        threads = [threading.Thread(target=run, args=(t,)) for t in range(8)]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
        assert not errs, errs
        for t in range(8):
            for got in out[t]:
                assert_same(got, alone_sparse if t % 2 else alone_dense)
        batches, calls = g.coalesce_stats()
        print(f"merged batches {batches}, calls in them {calls}")
        assert batches > 0 and calls >= 2 * batches
