"""nmn_hnsw_cache_search / _sparse / _device and the live mask (GpuHnsw.cache_search*, set_node_mask, node_live; docs/hnsw.md §16)
against tests/_cache_index_oracle.py: ids, order, counts and similarity BITS, except Angular / Geodesic, whose similarity is held to
2^-22 (one ulp of the raw acos, as tests/test_gpu_xmetric.py holds it)."""
import functools
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import _cache_index_oracle as co
from tests import _hnsw_mixed_oracle as mo
from tests import _hnsw_oracle as ho
from tests import _xmetric_oracle as xo

pytestmark = pytest.mark.gpu
F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "cache_index_small.npz")
ACOS = (xo.ANGULAR, xo.GEODESIC)
SIM_TOL = 2.0 ** -22
NINE = [xo.Metric(k) for k in range(8)] + [xo.Metric(xo.COMPOSITE, xo.GeometricConfig.default())]
NONE64 = np.uint64(0xFFFFFFFFFFFFFFFF)


def g_metric(m):
    from neumann_amd import ExtendedDistanceMetric, GeometricConfig
    if m.kind == xo.COMPOSITE:
        return ExtendedDistanceMetric.Composite(GeometricConfig(*[float(w) for w in m.config.weights()]))
    return ExtendedDistanceMetric(m.kind)


def g_config(cfg):
    from neumann_amd import HNSWConfig
    return HNSWConfig(m=cfg.m, m0=cfg.m0, ef_construction=cfg.ef_construction, ef_search=cfg.ef_search,
                      distance_metric=cfg.distance_metric)


def bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


def b1(x):
    return int(np.float32(x).view(np.uint32))


def host(out):
    import torch
    torch.cuda.synchronize()
    ids, sc, cnt = out
    return ids.cpu().numpy().view(np.uint64), sc.cpu().numpy(), cnt.cpu().numpy().view(np.uint32)


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=F)).cuda()


def assert_answers(metric, got, want_results, k, what):
    """got: the library's (ids, sims, counts[, stats]); want_results: the oracle's [(node, sim)] per query"""
    ids, sc, cnt = got[:3]
    wi, ws, wc = co.padded(want_results, k)
    assert cnt.tolist() == wc.tolist(), (what, "counts", cnt.tolist(), wc.tolist())
    assert np.array_equal(ids, wi), (what, "ids", np.argwhere(ids != wi)[:4].tolist())
    if metric.kind in ACOS:
        used = wi != NONE64
        assert np.abs(sc[used].astype(np.float64) - ws[used].astype(np.float64)).max(initial=0.0) <= SIM_TOL, what
        assert np.array_equal(bits(sc[~used]), bits(ws[~used])), what
    else:
        assert np.array_equal(bits(sc), bits(ws)), (what, "similarity bits", np.argwhere(bits(sc) != bits(ws))[:4].tolist())


def build_pair(items, cfg, dim):
    """items: a row (Dense) or a SparseVector (Sparse) per node, inserted in order into the oracle and, run by run, the library"""
    from neumann_amd import GpuHnsw
    o = mo.HNSWMixedIndex(cfg)
    g = GpuHnsw(dim, g_config(cfg))
    i = 0
    while i < len(items):
        j = i
        sparse = isinstance(items[i], mo.SparseVector)
        while j < len(items) and isinstance(items[j], mo.SparseVector) == sparse:
            j += 1
        for it in items[i:j]:
            o.insert_sparse(it) if sparse else o.insert(it)
        if sparse:
            g.insert_sparse(*mo.csr_of(items[i:j]))
        else:
            g.insert(np.stack(items[i:j]))
        i = j
    return o, g


def with_duplicate(rng, sv):
    p = sv.positions[int(rng.integers(len(sv)))]
    return mo.SparseVector.from_parts(sv.dimension, sv.positions + [p], np.append(sv.values, F(rng.standard_normal())))


# ---- the golden file through all three entries -------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def golden():
    from neumann_amd import GpuHnsw
    g = np.load(GOLDEN)
    dim = g["rows"].shape[1]
    nodes = mo.vectors_from_csr(dim, g["node_indptr"], g["node_pos"], g["node_val"])
    h = GpuHnsw(dim)
    it = iter(nodes)
    for i in range(g["rows"].shape[0]):   # one by one: Dense and Sparse alternate
        if g["sparse_mask"][i]:
            h.insert_sparse(*mo.csr_of([next(it)]))
        else:
            h.insert(g["rows"][i])
    h.set_node_mask(np.flatnonzero(~g["live"]), False)
    return g, h


def golden_want(g, form, k, mi):
    ids, sims, cnt = g[f"{form}_k{k}_ids"][mi], g[f"{form}_k{k}_sims"][mi], g[f"{form}_k{k}_counts"][mi]
    return [[(int(ids[q, j]), sims[q, j]) for j in range(cnt[q])] for q in range(ids.shape[0])]


@pytest.mark.parametrize("k", [1, 4, 10])
def test_golden_through_the_three_entries(k):
    g, h = golden()
    assert [h.node_live(i) for i in range(400)] == g["live"].tolist() and h.node_live(400) is None
    Q = g["dense_queries"]
    for mi, metric in enumerate(NINE):
        gm = g_metric(metric)
        for form, thr in (("dense", g["dense_thresholds"][mi]), ("sparse", g["sparse_thresholds"][mi])):
            want = golden_want(g, form, k, mi)
            for q in range(Q.shape[0]):   # a threshold per (metric, query): one call each, and the coalescer's uniform chain
                if form == "dense":
                    got = h.cache_search(Q[q], k, thr[q], gm, with_stats=True)
                    assert got[3].candidates_rescored == max(3 * k, 10)
                    if q % 8 == 0:
                        assert_answers(metric, host(h.cache_search_device(dev(Q[q]), k, float(thr[q]), gm)), want[q:q + 1], k,
                                       f"golden device {metric} k={k} q={q}")
                else:
                    a, b = int(g["sq_indptr"][q]), int(g["sq_indptr"][q + 1])
                    got = h.cache_search_sparse([0, b - a], g["sq_pos"][a:b], g["sq_val"][a:b], k, thr[q], gm)
                assert_answers(metric, got, want[q:q + 1], k, f"golden {form} {metric} k={k} q={q}")


def test_golden_sort_path_in_a_child_process(tmp_path):
    """NMN_XMETRIC_SORT_FROM=8: every call with more than 8 candidates is ordered by the filtered prep kernel and the large-k sort;
    a fresh process, against this one's rank path, bit for bit"""
    g, h = golden()
    out = tmp_path / "sorted.npz"
    script = tmp_path / "child.py"
    script.write_text(
        "import sys, numpy as np\n"
        f"sys.path.insert(0, {ROOT!r})\n"
        "from tests import test_gpu_hnsw_cache_search as t\n"
        "g, h = t.golden()\n"
        "res = {}\n"
        "for mi in (0, 3, 6, 8):\n"
        "    gm = t.g_metric(t.NINE[mi])\n"
        "    for q in range(0, 64, 4):\n"
        "        for k in (1, 10):\n"
        "            i, s, c = h.cache_search(g['dense_queries'][q], k, g['dense_thresholds'][mi][q], gm)\n"
        "            res[f'd{mi}_{q}_{k}_i'], res[f'd{mi}_{q}_{k}_s'], res[f'd{mi}_{q}_{k}_c'] = i, s, c\n"
        "            a, b = int(g['sq_indptr'][q + 1]), int(g['sq_indptr'][q + 2])\n"
        "            i, s, c = h.cache_search_sparse([0, b - a], g['sq_pos'][a:b], g['sq_val'][a:b], k, g['sparse_thresholds'][mi][q + 1], gm)\n"
        "            res[f's{mi}_{q}_{k}_i'], res[f's{mi}_{q}_{k}_s'], res[f's{mi}_{q}_{k}_c'] = i, s, c\n"
        "            i, s, c = t.host(h.cache_search_device(t.dev(g['dense_queries'][q]), k, float(g['dense_thresholds'][mi][q]), gm))\n"
        "            res[f'v{mi}_{q}_{k}_i'], res[f'v{mi}_{q}_{k}_s'], res[f'v{mi}_{q}_{k}_c'] = i, s, c\n"
        f"np.savez({str(out)!r}, **res)\n")
    env = dict(os.environ, NMN_XMETRIC_SORT_FROM="8")
    r = subprocess.run([sys.executable, str(script)], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    got = np.load(out)
    for mi in (0, 3, 6, 8):
        gm = g_metric(NINE[mi])
        for q in range(0, 64, 4):
            for k in (1, 10):
                a, b = int(g["sq_indptr"][q + 1]), int(g["sq_indptr"][q + 2])
                mine = {"d": h.cache_search(g["dense_queries"][q], k, g["dense_thresholds"][mi][q], gm),
                        "s": h.cache_search_sparse([0, b - a], g["sq_pos"][a:b], g["sq_val"][a:b], k, g["sparse_thresholds"][mi][q + 1], gm)}
                mine["v"] = mine["d"]
                for tag, (i, s, c) in mine.items():
                    key = f"{tag}{mi}_{q}_{k}"
                    assert np.array_equal(got[key + "_i"], i) and np.array_equal(got[key + "_c"], c), key
                    assert np.array_equal(bits(got[key + "_s"]), bits(s)), key


# ---- three HNSW metrics x nine re-rank metrics x dimensions x node kinds ----------------------------------------------------------
SMALL = dict(m=8, ef_construction=48, ef_search=24)
SMALL_LONG = dict(m=6, ef_construction=20, ef_search=24)   # the long rows: the oracle's build is what a case costs
N_NODES = 300


@functools.lru_cache(maxsize=None)
def shaped(hnsw_metric, dim, kinds):
    rng = np.random.default_rng(7919 * dim + 31 * hnsw_metric + len(kinds))
    rows = rng.standard_normal((N_NODES, dim)).astype(F)
    rows[rng.random(rows.shape) < (0.55 if dim > 8 else 0.3)] = 0.0
    rows[17] = 0.0                       # a zero row
    rows[40] = rows[39]                  # duplicate rows: ties keep the walk's order
    rows[41] = rows[39]
    counts = [0, 1, 7, 8, 9, dim]        # stored entries of the first Sparse nodes
    items, n_sparse = [], 0
    for i in range(N_NODES):
        sparse = kinds == "sparse" or (kinds == "mixed" and i % 2 == 1)
        if not sparse:
            items.append(rows[i])
            continue
        if n_sparse < len(counts):
            nnz = min(counts[n_sparse], dim)
            v = np.zeros(dim, dtype=F)
            v[rng.permutation(dim)[:nnz]] = rng.standard_normal(nnz).astype(F) + F(3.0)
            sv = mo.SparseVector.from_dense(v)
        else:
            sv = mo.SparseVector.from_dense(rows[i])
            if n_sparse % 9 == 4 and len(sv):
                sv = with_duplicate(rng, sv)
        n_sparse += 1
        items.append(sv)
    cfg = ho.HNSWConfig(**(SMALL_LONG if dim > 100 else SMALL)).with_distance_metric(hnsw_metric)
    o, g = build_pair(items, cfg, dim)
    dead = np.flatnonzero(rng.random(N_NODES) < 0.15)
    g.set_node_mask(dead, False)
    live = np.ones(N_NODES, dtype=bool)
    live[dead] = False
    Q = rng.standard_normal((6, dim)).astype(F)
    Q[1, rng.random(dim) < 0.6] = 0.0
    Q[2] = rows[39]                      # finds the three duplicate rows
    Q[3] = 0.0                           # a zero query
    sq = [mo.SparseVector.from_dense(Q[1]), mo.SparseVector.from_dense(Q[4])]
    if len(sq[0]):
        sq.append(with_duplicate(rng, sq[0]))
    return o, g, live, Q, sq


@pytest.mark.parametrize("kinds", ["dense", "sparse", "mixed"])
@pytest.mark.parametrize("dim", [5, 8, 20, 33, 771])
@pytest.mark.parametrize("hnsw_metric", [ho.COSINE, ho.EUCLIDEAN, ho.DOT_PRODUCT])
def test_shapes_metrics_and_node_kinds(hnsw_metric, dim, kinds):
    o, g, live, Q, sq = shaped(hnsw_metric, dim, kinds)
    is_live = lambda n: bool(live[n])  # noqa: E731
    for mi, metric in enumerate(NINE):
        gm = g_metric(metric)
        k = (1, 4, 7)[mi % 3]
        # the threshold: the similarity BITS of one of the query's candidates (equality passes); -inf where acos decides
        for qi in range(Q.shape[0]):
            cands = [n for n, _ in o.search(Q[qi], co.candidate_count(k))]
            all_of = co.rescore(o, is_live, cands, xo.Sparse(Q[qi]), len(cands), -math.inf, metric)   # every live candidate, in order
            thr = -math.inf if metric.kind in ACOS or not all_of else float(all_of[len(all_of) // 2][1])
            want = [e for e in all_of if e[1] >= F(thr)][:k]
            what = f"hnsw={hnsw_metric} d={dim} {kinds} {metric} k={k} q={qi} thr={thr}"
            assert_answers(metric, g.cache_search(Q[qi], k, thr, gm), [want], k, what)
            if qi in (0, 2):
                assert_answers(metric, host(g.cache_search_device(dev(Q[qi]), k, thr, gm)), [want], k, "device " + what)
        for si, s in enumerate(sq):   # sparse queries: walked on the device or, per §15, on the host; one holds a duplicate
            thr = -math.inf if metric.kind in ACOS else 0.2
            want = co.search_nodes_sparse(o, is_live, s, k, thr, metric)
            assert_answers(metric, g.cache_search_sparse(*mo.csr_of([s]), k, thr, gm), [want], k,
                           f"sparse query {si} hnsw={hnsw_metric} d={dim} {kinds} {metric} k={k}")


def test_several_queries_in_one_call_and_the_stats():
    o, g, live, Q, sq = shaped(ho.COSINE, 20, "mixed")
    is_live = lambda n: bool(live[n])  # noqa: E731
    for metric in (NINE[0], NINE[5], NINE[8]):
        want = [co.search_nodes(o, is_live, q, 4, 0.3, metric) for q in Q]
        got = g.cache_search(Q, 4, 0.3, g_metric(metric), with_stats=True)
        assert_answers(metric, got, want, 4, f"6 queries {metric}")
        assert got[3].candidates_rescored == 12 and got[3].rows_scanned > 0
        assert_answers(metric, host(g.cache_search_device(dev(Q), 4, 0.3, g_metric(metric))), want, 4, f"6 queries device {metric}")
        wants = [co.search_nodes_sparse(o, is_live, s, 4, 0.3, metric) for s in sq]
        assert_answers(metric, g.cache_search_sparse(*mo.csr_of(sq), 4, 0.3, g_metric(metric)), wants, 4, f"3 sparse queries {metric}")


# ---- the merge kernel against the dense loop ---------------------------------------------------------------------------------------
def test_merge_kernel_equals_the_dense_loop_without_duplicates_and_differs_with_them():
    """all-Sparse handle, every node a candidate (k = n): on duplicate-free nodes the merge kernel's similarity is bit for bit
    score_rows_xmetric's over the to_dense() rows; on a node with a duplicated position it is the oracle's and NOT the dense loop's"""
    rng = np.random.default_rng(99)
    dim, n = 33, 40
    rows = rng.standard_normal((n, dim)).astype(F)
    rows[rng.random(rows.shape) < 0.6] = 0.0
    items = [mo.SparseVector.from_dense(r) for r in rows]
    dup = [3, 11, 27]
    for i in dup:
        items[i] = with_duplicate(rng, items[i])
    o, g = build_pair(items, ho.HNSWConfig(**SMALL), dim)
    q = rng.standard_normal(dim).astype(F)
    differs = 0
    for metric in NINE:
        if metric.kind in ACOS:
            continue
        ids, sims, cnt = g.cache_search(q, n, -math.inf, g_metric(metric))
        assert cnt[0] == n
        _, dense_sims = g.vectors().score_rows_xmetric(q, ids[0], g_metric(metric))
        for j, node in enumerate(ids[0].tolist()):
            want = co.similarity(metric, xo.Sparse(q), co.stored_entries(o, node))
            assert b1(sims[0, j]) == b1(want), (metric, node)
            if node not in dup:
                assert b1(sims[0, j]) == b1(dense_sims[0, j]), (metric, node)
            else:
                differs += int(b1(sims[0, j]) != b1(dense_sims[0, j]))
    assert differs >= len(dup) * 4     # (most metrics see the first duplicate where the dense row holds the last)


# ---- the mask ------------------------------------------------------------------------------------------------------------------------
def test_mask_all_dead_flipped_and_new_nodes():
    rng = np.random.default_rng(5)
    dim = 8
    rows = rng.standard_normal((40, dim)).astype(F)
    o, g = build_pair(list(rows), ho.HNSWConfig(**SMALL), dim)
    metric, gm = NINE[0], g_metric(NINE[0])
    g.set_node_mask(np.arange(40), False)
    ids, sims, cnt = g.cache_search(rows[:3], 5, -math.inf, gm)
    assert cnt.tolist() == [0, 0, 0] and (ids == NONE64).all() and np.isneginf(sims).all()
    plain = g.search(rows[:3], 5)                       # every other entry ignores the mask
    wi, ws, wc = mo.answers_dense(o, rows[:3], 5)
    assert np.array_equal(plain[0], wi) and np.array_equal(bits(plain[1]), bits(ws))
    live = np.zeros(41, dtype=bool)
    g.set_node_mask([4, 5, 36, 4], True)
    live[[4, 5, 36]] = True
    want = [co.search_nodes(o, lambda n: bool(live[n]), q, 5, -math.inf, metric) for q in rows[3:6]]
    assert_answers(metric, g.cache_search(rows[3:6], 5, -math.inf, gm), want, 5, "three live")
    extra = rng.standard_normal(dim).astype(F)
    assert o.insert(extra) == 40 and g.insert(extra).tolist() == [40]
    live[40] = True                                     # a node inserted after the flips is live, and the flips stay
    assert g.node_live(40) is True and g.node_live(0) is False and g.node_live(4) is True
    want = [co.search_nodes(o, lambda n: bool(live[n]), q, 5, -math.inf, metric) for q in (extra, rows[4])]
    assert_answers(metric, g.cache_search(np.stack([extra, rows[4]]), 5, -math.inf, gm), want, 5, "after an insert")
    assert want[0][0][0] == 40
    from neumann_amd import _capi
    with pytest.raises(_capi.NeumannGpuError):
        g.set_node_mask([3, 41], False)                 # a node the index does not hold: nothing flipped
    assert g.node_live(3) is False and g.node_live(41) is None


def test_hbm_bytes_counts_the_mask():
    """one insert call on a fresh handle: every device buffer is allocated once, for bytes + bytes / 4 (at least 256, nothing for no
    bytes), so nmn_hnsw_hbm_bytes can be added up — the flat index, the five adjacency arrays, and the mask's (n + 31) / 32 words"""
    from neumann_amd import GpuHnsw, HNSWConfig, synth_rows
    n, dim, m = 3000, 8, 8
    with GpuHnsw(dim, HNSWConfig(m=m, ef_construction=24, ef_search=16)) as g:
        g.insert(synth_rows(0x5EED0051, 0, n, dim))
        levels = g.levels()
        n_upper, L = int((levels > 0).sum()), max(g.max_layer, 1)
        cap = lambda b: max(b + b // 4, 256) if b else 0  # noqa: E731
        adjacency = cap(n * 2 * m * 4) + cap(n * 4) + cap(n * 4) + cap(n_upper * L * m * 4) + cap(n_upper * L * 4)
        mask = cap((n + 31) // 32 * 4)
        assert mask == 470 and n_upper > 0
        assert g.hbm_bytes == sum(g.vectors().hbm_bytes()) + adjacency + mask


def test_thresholds_inf_nan_and_the_overflow_paths():
    o, g, live, Q, sq = shaped(ho.COSINE, 20, "mixed")
    is_live = lambda n: bool(live[n])  # noqa: E731
    metric, gm = NINE[6], g_metric(NINE[6])
    for thr in (-math.inf, math.inf, math.nan):
        want = [co.search_nodes(o, is_live, q, 4, thr, metric) for q in Q]
        assert_answers(metric, g.cache_search(Q, 4, thr, gm), want, 4, f"thr={thr}")
        if thr != -math.inf:
            assert all(w == [] for w in want)
    want = [co.search_nodes(o, is_live, q, 7, 0.1, metric) for q in Q]
    try:
        for rcap, ccap in ((4, 0), (0, 4), (4, 4)):   # the results heap, the candidate heap, both outgrow LDS: the spill launch
            g.set_heap_capacity(rcap, ccap)
            got = g.cache_search(Q, 7, 0.1, gm, with_stats=True)
            assert_answers(metric, got, want, 7, f"heaps {rcap}/{ccap}")
            assert got[3].fallback_queries > 0
            assert_answers(metric, host(g.cache_search_device(dev(Q), 7, 0.1, gm)), want, 7, f"device heaps {rcap}/{ccap}")
    finally:
        g.set_heap_capacity(0, 0)


# ---- refusals, empty and tiny indexes ------------------------------------------------------------------------------------------------
def test_refusals_write_nothing():
    from neumann_amd import ExtendedDistanceMetric, GpuHnsw, _capi
    rows = np.random.default_rng(2).standard_normal((20, 6)).astype(F)
    lib = _capi.load()
    import ctypes as C

    def raw_call(h, k, kind):
        ids = np.full(8, 77, dtype=np.uint64)
        sc = np.full(8, 7.0, dtype=F)
        cnt = np.full(1, 9, dtype=np.uint32)
        m = _capi.XMetric(kind, 0.0, 0.0, 0.0)
        st = lib.nmn_hnsw_cache_search(h._h, C.c_void_p(rows.ctypes.data), 1, k, 0.0, C.byref(m), C.c_void_p(ids.ctypes.data),
                                       C.c_void_p(sc.ctypes.data), C.c_void_p(cnt.ctypes.data), None)
        assert (ids == 77).all() and (sc == 7.0).all() and cnt[0] == 9
        return st

    def raw_sparse(h, indptr, positions, values):
        """nmn_hnsw_cache_search_sparse on poisoned outputs: the status, with nothing written"""
        ip, pos, val = np.asarray(indptr, np.uint64), np.asarray(positions, np.uint32), np.asarray(values, F)
        ids = np.full(8, 77, dtype=np.uint64)
        sc = np.full(8, 7.0, dtype=F)
        cnt = np.full(2, 9, dtype=np.uint32)
        m = _capi.XMetric(0, 0.0, 0.0, 0.0)
        st = lib.nmn_hnsw_cache_search_sparse(h._h, C.c_void_p(ip.ctypes.data), C.c_void_p(pos.ctypes.data), C.c_void_p(val.ctypes.data),
                                              ip.size - 1, 3, 0.0, C.byref(m), C.c_void_p(ids.ctypes.data), C.c_void_p(sc.ctypes.data),
                                              C.c_void_p(cnt.ctypes.data), None)
        assert (ids == 77).all() and (sc == 7.0).all() and (cnt == 9).all()
        return st
    with GpuHnsw(6, storage="quantized") as q8:
        q8.insert(rows)
        assert raw_call(q8, 3, 0) == _capi.ERR_CONFIGURATION
        assert raw_sparse(q8, [0, 1], [0], [1.0]) == _capi.ERR_CONFIGURATION
        with pytest.raises(_capi.NeumannGpuError):
            q8.cache_search_sparse([0, 1], [0], [1.0], 3, 0.0, ExtendedDistanceMetric.Cosine)
    with GpuHnsw(6) as g:
        g.insert(rows)
        assert raw_call(g, 0, 0) == _capi.ERR_INVALID_TOP_K
        assert raw_call(g, 3, 9) == _capi.ERR_CONFIGURATION and raw_call(g, 3, -1) == _capi.ERR_CONFIGURATION
        assert raw_sparse(g, [0, 1, 2], [0, 6], [1.0, 1.0]) == _capi.ERR_INVALID_ARGUMENT   # the SECOND query is bad: the first unanswered
        assert raw_sparse(g, [0, 2, 1], [0, 1], [1.0, 1.0]) == _capi.ERR_INVALID_ARGUMENT   # indptr decreases
        with pytest.raises(_capi.NeumannGpuError) as e:
            g.cache_search_sparse([0, 1], [6], [1.0], 3, 0.0, ExtendedDistanceMetric.Cosine)
        assert "index 6 out of bounds for dimension 6" in str(e.value)
        with pytest.raises(_capi.NeumannGpuError):
            g.cache_search_sparse([1, 0], [0], [1.0], 3, 0.0, ExtendedDistanceMetric.Cosine)


def test_empty_and_single_node():
    from neumann_amd import ExtendedDistanceMetric as M, GpuHnsw
    with GpuHnsw(5) as g:
        q = np.ones((2, 5), dtype=F)
        for out in (g.cache_search(q, 3, -math.inf, M.Cosine), g.cache_search_sparse([0, 1, 2], [0, 1], [1.0, 1.0], 3, -math.inf, M.Cosine),
                    host(g.cache_search_device(dev(q), 3, -math.inf, M.Cosine))):
            assert out[2].tolist() == [0, 0] and (out[0] == NONE64).all()
        g.insert(np.arange(5, dtype=F))
        o = mo.HNSWMixedIndex()
        o.insert(np.arange(5, dtype=F))
        for metric in NINE:
            want = [co.search_nodes(o, lambda n: True, x, 3, -math.inf, metric) for x in q]
            assert_answers(metric, g.cache_search(q, 3, -math.inf, g_metric(metric)), want, 3, f"n=1 {metric}")
            assert want[0][0][0] == 0


def test_existing_entries_ignore_dead_nodes():
    o, g, live, Q, sq = shaped(ho.COSINE, 20, "mixed")
    from neumann_amd import ExtendedDistanceMetric as M
    assert not live.all()
    wi, ws, wc = mo.answers_dense(o, Q, 10)
    for got in (g.search(Q, 10), host(g.search_device(dev(Q), 10)), g.search_multi(Q, [10] * len(Q))):
        assert np.array_equal(got[0], wi) and np.array_equal(bits(got[1]), bits(ws)) and got[2].tolist() == wc.tolist()
    assert (~live[wi[wi != NONE64].astype(np.int64)]).any()      # (dead nodes are among these answers)
    si, ss, sc = mo.answers_sparse(o, sq, 10)
    got = g.search_sparse(*mo.csr_of(sq), 10)
    assert np.array_equal(got[0], si) and np.array_equal(bits(got[1]), bits(ss))
    # the metric entries: search_with_hnsw_and_metric over the to_dense() rows of ALL nodes, dead ones included — ids, counts, score bits
    def metric_want(q, top_k, metric):
        return xo.rerank(metric, q, [n for n, _ in o.search(q, xo.candidate_count(top_k))], lambda n: (n, o.rows[n]), top_k)

    def held(got, want, k, what):
        wi, ws, wc = co.padded(want, k)
        assert np.array_equal(got[0], wi) and got[2].tolist() == wc.tolist(), what
        assert np.array_equal(bits(got[1]), bits(ws)), what
        assert (~live[wi[wi != NONE64].astype(np.int64)]).any(), what     # (dead nodes are among these answers too)

    plain = [NINE[i] for i in (0, 3, 5, 6, 7, 8)]                         # (the metrics held to bits: no acos)
    for metric in plain:
        want = [metric_want(q, 5, metric) for q in Q]
        held(g.search_metric(Q, 5, g_metric(metric)), want, 5, f"search_metric {metric}")
        held(host(g.search_metric_device(dev(Q), 5, g_metric(metric))), want, 5, f"search_metric_device {metric}")
    tops = [1, 5, 7, 3, 10, 2]
    want = [metric_want(q, t, m) for q, t, m in zip(Q, tops, plain)]
    held(g.search_metric_multi(Q, tops, [g_metric(m) for m in plain], kstride=10), want, 10, "search_metric_multi")
    ks = [10, 3, 7][:len(sq)]
    want = [o.search_sparse_with_ef(s, k, o.config.ef_search) for s, k in zip(sq, ks)]
    held(g.search_sparse_multi(*mo.csr_of(sq), ks, kstride=10), want, 10, "search_sparse_multi")
