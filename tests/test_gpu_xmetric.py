"""The extended distance metrics on the GPU (neumann_amd/csrc/nmn_xmetric.hip) against tests/_xmetric_oracle.py:
GpuFlatIndex.score_rows_xmetric (the kernel alone) and GpuHnsw.search_metric / search_metric_device (walk + re-rank + stable
ordering).  Raw values, similarities and answers are held to the oracle's BITS for the seven metrics without acos; Angular and
Geodesic to one ulp of the raw value and 2^-22 of the similarity (one ulp of a value in [2, 4) is 2^-22; divided by pi, plus two
roundings below 2^-24 each, the similarity stays under that)."""
import functools
import os

import numpy as np
import pytest

from tests import _hnsw_oracle as ho
from tests import _xmetric_oracle as xo

pytestmark = pytest.mark.gpu
F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "hnsw_small.npz")
ACOS = (xo.ANGULAR, xo.GEODESIC)
SIM_TOL = 2.0 ** -22

# (id, oracle metric): the eight unit variants and Composite with default, structural_heavy, (0, 0, 0) and (1, 0, 0)
METRICS = [(xo.NAMES[k], xo.Metric(k)) for k in range(8)] + [
    ("Composite-default", xo.Metric(xo.COMPOSITE, xo.GeometricConfig.default())),
    ("Composite-structural_heavy", xo.Metric(xo.COMPOSITE, xo.GeometricConfig.structural_heavy())),
    ("Composite-0-0-0", xo.Metric(xo.COMPOSITE, xo.GeometricConfig(0.0, 0.0, 0.0))),
    ("Composite-1-0-0", xo.Metric(xo.COMPOSITE, xo.GeometricConfig(1.0, 0.0, 0.0))),
]
NINE = METRICS[:9]


def g_metric(m):
    from neumann_amd import ExtendedDistanceMetric, GeometricConfig
    if m.kind == xo.COMPOSITE:
        return ExtendedDistanceMetric.Composite(GeometricConfig(*[float(w) for w in m.config.weights()]))
    return ExtendedDistanceMetric(m.kind)


def bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


def assert_scores(metric, got_raw, got_sim, want_raw, want_sim, what):
    if metric.kind in ACOS:
        ulps = np.abs(bits(got_raw).astype(np.int64) - bits(want_raw).astype(np.int64))  # (acos is >= +0.0: bit order is value order)
        print(f"{what}: acos raw max ulp distance {ulps.max()}, similarity max |diff| {np.abs(got_sim - want_sim).max():.3e}")
        assert ulps.max() <= 1, what
        assert np.abs(got_sim.astype(np.float64) - want_sim.astype(np.float64)).max() <= SIM_TOL, what
    else:
        bad = np.argwhere(bits(got_raw) != bits(want_raw))
        assert bad.size == 0, (what, "raw", bad[:5], got_raw[tuple(bad[0])], want_raw[tuple(bad[0])])
        bad = np.argwhere(bits(got_sim) != bits(want_sim))
        assert bad.size == 0, (what, "similarity", bad[:5], got_sim[tuple(bad[0])], want_sim[tuple(bad[0])])


# ---- the kernel alone: score_rows_xmetric -------------------------------------------------------------------------------------
DIMS = [1, 7, 8, 9, 37, 768]  # the group tail, the chunk tail, one long row
CORPORA = ["dense", "sparse60", "zero", "negzero", "scaled", "huge"]
LIST9 = [63, 0, 5, 5, 17, 32, 45, 1, 62]  # nine rows: the second wave of pairs is partly filled


@functools.lru_cache(maxsize=None)
def kernel_corpus(kind, dim):
    rng = np.random.default_rng(1000 * dim + sum(map(ord, kind)))
    R = rng.standard_normal((64, dim)).astype(F)
    Q = rng.standard_normal((3, dim)).astype(F)
    if kind == "sparse60":       # 60 % of the entries zeroed
        R[rng.random(R.shape) < 0.6] = 0.0
        Q[rng.random(Q.shape) < 0.6] = 0.0
    elif kind == "zero":         # a zero row and a zero query
        R[5] = 0.0
        Q[1] = 0.0
    elif kind == "negzero":      # -0.0 must count as not stored
        R[rng.random(R.shape) < 0.3] = -0.0
        Q[rng.random(Q.shape) < 0.3] = -0.0
        R[7] = -0.0
    elif kind == "scaled":       # rows scaled by 1e30 and 1e-30
        R[0::2] *= F(1e30)
        R[1::2] *= F(1e-30)
        Q[1] *= F(1e30)
        Q[2] *= F(1e-30)
    elif kind == "huge":         # the clamp of Euclidean / Manhattan at f32::MAX fires
        R[0] = F(3e38)
        R[1] = F(-3e38)
        R[2, ::2] = F(3e38)
    return R, Q


@functools.lru_cache(maxsize=None)
def kernel_reference(kind, dim, mid):
    R, Q = kernel_corpus(kind, dim)
    metric = dict(METRICS)[mid]
    return xo.score_matrix(metric, Q, R)


@pytest.mark.parametrize("kind", CORPORA)
@pytest.mark.parametrize("dim", DIMS)
def test_score_rows_equals_oracle(dim, kind):
    from neumann_amd import GpuFlatIndex
    R, Q = kernel_corpus(kind, dim)
    all_rows = np.arange(64, dtype=np.uint64)
    idx = GpuFlatIndex(dim, 64)
    idx.upload(R)
    for mid, metric in METRICS:
        want_raw, want_sim = kernel_reference(kind, dim, mid)
        gm = g_metric(metric)
        raw, sim = idx.score_rows_xmetric(Q, all_rows, gm)              # 3 queries x 64 rows
        assert_scores(metric, raw, sim, want_raw, want_sim, f"{mid} {kind} d={dim} 3x64")
        raw, sim = idx.score_rows_xmetric(Q[0], all_rows, gm)           # 1 query
        assert_scores(metric, raw, sim, want_raw[:1], want_sim[:1], f"{mid} {kind} d={dim} 1x64")
        raw, sim = idx.score_rows_xmetric(Q, LIST9, gm)                 # a list of 9 rows
        assert_scores(metric, raw, sim, want_raw[:, LIST9], want_sim[:, LIST9], f"{mid} {kind} d={dim} 3x9")
        raw, sim = idx.score_rows_xmetric(Q[2], LIST9, gm)
        assert_scores(metric, raw, sim, want_raw[2:, LIST9], want_sim[2:, LIST9], f"{mid} {kind} d={dim} 1x9")
    if kind == "huge" and dim >= 2:  # (the case is what it says)
        assert kernel_reference(kind, dim, "Euclidean")[0][0, 0] == np.finfo(F).max
        assert kernel_reference(kind, dim, "Manhattan")[0][0, 1] == np.finfo(F).max


@pytest.mark.parametrize("dim", [9, 37])
def test_nan_components_structure_only(dim):
    """NaN is stored by from_dense: it counts for Jaccard / Overlap, and Cosine sanitises it to 0.0"""
    from neumann_amd import GpuFlatIndex
    rng = np.random.default_rng(dim)
    R = rng.standard_normal((16, dim)).astype(F)
    R[rng.random(R.shape) < 0.5] = 0.0
    Q = rng.standard_normal((2, dim)).astype(F)
    Q[rng.random(Q.shape) < 0.5] = 0.0
    R[3, 0] = np.nan
    R[4, dim - 1] = np.nan
    Q[1, 2] = np.nan
    with GpuFlatIndex(dim, 16) as idx:
        idx.upload(R)
        for kind in (xo.COSINE, xo.JACCARD, xo.OVERLAP):
            metric = xo.Metric(kind)
            want_raw, want_sim = xo.score_matrix(metric, Q, R)
            raw, sim = idx.score_rows_xmetric(Q, np.arange(16), g_metric(metric))
            assert_scores(metric, raw, sim, want_raw, want_sim, f"NaN {metric} d={dim}")
            if kind == xo.COSINE:
                assert raw[0, 3] == 0.0 and raw[1, 0] == 0.0


@pytest.mark.parametrize("dim", [9, 37, 9000])
def test_score_host_rows_equals_oracle(dim):
    """nmn_xmetric_score_host_rows (the engine's changed path): rows in host memory, no index — 9 000 elements is longer than an
    index row may be; 11 rows leave the second wave partly filled"""
    from neumann_amd.xmetric import score_host_rows
    rng = np.random.default_rng(dim + 5)
    R = rng.standard_normal((11, dim)).astype(F)
    R[rng.random(R.shape) < (0.6 if dim < 100 else 0.97)] = 0.0
    R[4] = 0.0
    q = rng.standard_normal(dim).astype(F)
    q[rng.random(dim) < (0.5 if dim < 100 else 0.97)] = 0.0
    for mid, metric in NINE:
        want_raw, want_sim = xo.score_matrix(metric, q[None, :], R)
        raw, sim = score_host_rows(q, R, g_metric(metric))
        assert_scores(metric, raw[None, :], sim[None, :], want_raw, want_sim, f"host rows {mid} d={dim}")


def test_score_rows_argument_errors():
    from neumann_amd import ExtendedDistanceMetric, GpuFlatIndex, NeumannGpuError, _capi
    with GpuFlatIndex(4, 8) as idx:
        idx.upload(np.ones((3, 4), dtype=F))
        with pytest.raises(NeumannGpuError) as e:
            idx.score_rows_xmetric(np.ones(4, F), [0], ExtendedDistanceMetric(9))
        assert e.value.status == _capi.ERR_CONFIGURATION
        with pytest.raises(NeumannGpuError) as e:
            idx.score_rows_xmetric(np.ones(4, F), [3], ExtendedDistanceMetric.Cosine)
        assert e.value.status == _capi.ERR_NOT_FOUND


# ---- walk + re-rank -------------------------------------------------------------------------------------------------------------
GOLDENS = {"dense": GOLDEN, "sparse": os.path.join(ROOT, "tests", "golden", "hnsw_small_sparse.npz")}


@functools.lru_cache(maxsize=None)
def walk_corpus(name):
    rows, queries = ho.golden_corpus() if name == "dense" else xo.sparse_golden_corpus()  # sparse: 60 % of the entries zeroed
    return rows, queries[:33]


@functools.lru_cache(maxsize=None)
def walk_oracle(name):
    """the oracle's index of the corpus as its golden file records it (written from the oracle alone: tests/golden/make_golden_hnsw.py,
    make_golden_hnsw_sparse.py); the oracle walks it with its own arithmetic"""
    idx = xo.index_from_golden(GOLDENS[name])
    assert np.array_equal(idx.rows, walk_corpus(name)[0])
    return idx


@functools.lru_cache(maxsize=None)
def walk_sparse_rows(name):
    return [xo.Sparse(r) for r in walk_corpus(name)[0]]


@functools.lru_cache(maxsize=None)
def walk_candidates(name, c):
    """the walk's candidate ids per query, in its order: index.search(query, c)"""
    o = walk_oracle(name)
    return [[nid for nid, _ in o.search(q, c)] for q in walk_corpus(name)[1]]


@functools.lru_cache(maxsize=None)
def walk_gpu(name):
    from neumann_amd import GpuHnsw
    rows, _ = walk_corpus(name)
    g = GpuHnsw(rows.shape[1])
    g.insert(rows)
    return g


def walk_reference(name, metric, top_k):
    """-> ids, scores, counts in the library's layout, and per query [(id, cosine f32, similarity f32)] of every candidate"""
    rows, Q = walk_corpus(name)
    sparse = walk_sparse_rows(name)
    cands = walk_candidates(name, xo.candidate_count(top_k))
    ids = np.full((len(Q), top_k), np.uint64(0xFFFFFFFFFFFFFFFF), dtype=np.uint64)
    sc = np.full((len(Q), top_k), -np.inf, dtype=F)
    cnt = np.zeros(len(Q), dtype=np.uint32)
    lists = []
    for i, q in enumerate(Q):
        qs = xo.Sparse(q)
        scored = [(nid, xo.to_similarity(metric, xo.compute(metric, qs, sparse[nid]))) for nid in cands[i]]
        if metric.kind in ACOS:
            lists.append([(nid, xo.cosine_similarity(qs, sparse[nid]), s) for nid, s in scored])
        res = sorted(scored, key=lambda t: -float(t[1]))[:top_k]  # stable, descending (lib.rs:2611-2617)
        cnt[i] = len(res)
        for j, (nid, s) in enumerate(res):
            ids[i, j] = nid
            sc[i, j] = s
    return ids, sc, cnt, lists


def dev(Q):
    import torch
    return torch.from_numpy(np.ascontiguousarray(np.atleast_2d(Q), dtype=F)).cuda()


def host(res):
    ids, sc, counts = res
    return ids.cpu().numpy().view(np.uint64), sc.cpu().numpy(), counts.cpu().numpy().astype(np.uint32)


def assert_same_bits(got, want):
    assert np.array_equal(got[2], want[2]), (got[2], want[2])
    assert np.array_equal(got[0], want[0]), np.argwhere(got[0] != want[0])[:5]
    assert np.array_equal(bits(got[1]), bits(want[1])), np.argwhere(bits(got[1]) != bits(want[1]))[:5]


@pytest.mark.parametrize("name", ["dense", "sparse"])
@pytest.mark.parametrize("mid,metric", NINE, ids=[m[0] for m in NINE])
def test_search_metric_equals_oracle(mid, metric, name):
    rows, Q = walk_corpus(name)
    g = walk_gpu(name)
    gm = g_metric(metric)
    for top_k in (1, 5, 10, 500):  # c = 10, 10, 20, and 2 top_k > n
        if metric.kind in ACOS and top_k == 500:
            continue  # (the condition below is stated for top_k in {1, 5, 10}; test_acos_metrics_at_large_top_k covers 500)
        want_ids, want_sc, want_cnt, lists = walk_reference(name, metric, top_k)
        got = g.search_metric(Q, top_k, gm)                               # nq = 33, host buffers
        got_dev = host(g.search_metric_device(dev(Q), top_k, gm))         # the same on the device
        assert_same_bits(got_dev, got)
        one = g.search_metric(Q[0], top_k, gm)                            # nq = 1
        assert_same_bits(one, (got[0][:1], got[1][:1], got[2][:1]))
        if metric.kind in ACOS:
            # the comparison is meaningful only where one ulp of acos cannot reorder two candidates: no two of a list within 2^-21
            # of each other unless their f32 cosines are bit-identical (then both sides give them one score, whatever acos is)
            pairs = close = 0
            for lst in lists:
                for a in range(len(lst)):
                    for b in range(a + 1, len(lst)):
                        pairs += 1
                        if abs(float(lst[a][2]) - float(lst[b][2])) < 2.0 ** -21:
                            close += 1
                            assert lst[a][1].tobytes() == lst[b][1].tobytes(), (name, top_k, lst[a], lst[b])
            print(f"{mid} {name} top_k={top_k}: {pairs} candidate pairs, {close} within 2^-21 (identical cosines)")
            assert np.array_equal(got[2], want_cnt) and np.array_equal(got[0], want_ids)
            used = want_ids != np.uint64(0xFFFFFFFFFFFFFFFF)
            diff = np.abs(got[1][used].astype(np.float64) - want_sc[used].astype(np.float64))
            print(f"{mid} {name} top_k={top_k}: similarity max |diff| {diff.max():.3e}")
            assert diff.max() <= SIM_TOL
            assert np.all(np.isneginf(got[1][~used]))
        else:
            assert_same_bits(got, (want_ids, want_sc, want_cnt))
        if name == "dense" and metric.kind in (xo.JACCARD, xo.OVERLAP):
            # every score is 1.0: the answer is the walk's first top_k in the walk's order — the stable ordering
            c = xo.candidate_count(top_k)
            walk_ids = ho.padded_answers(walk_oracle(name), Q, min(c, len(rows)))[0][:, :top_k]
            assert np.all(got[2] == top_k) and np.all(got[1] == 1.0)
            assert np.array_equal(got[0], walk_ids)


@pytest.mark.parametrize("name", ["dense", "sparse"])
def test_the_walked_graph_is_the_oracles(name):
    """the graph nmn_hnsw_insert builds over the corpus is the golden file's, list by list"""
    g, o = walk_gpu(name), walk_oracle(name)
    assert len(g) == len(o) and g.entry_point == o.entry_point and g.max_layer == o.max_layer
    assert g.levels().tolist() == o.levels
    for node in range(len(o)):
        for layer in range(o.levels[node] + 1):
            assert g.neighbors(node, layer).tolist() == o.neighbors[node][layer], (node, layer)


@pytest.mark.parametrize("kind", ACOS)
def test_acos_metrics_at_large_top_k(kind):
    """top_k = 500 (every node a candidate) under Angular / Geodesic, where the condition of the small top_k does not hold for every
    pair: every score is within 2^-22 of the oracle's score for that id, the ids are a permutation of the oracle's first 500 apart
    from what sits within 2^-21 of the 500th score, and position by position the id is the oracle's wherever the oracle's score
    there is at least 2^-21 away from both of its neighbours' (one ulp of acos cannot move such an entry)"""
    metric = xo.Metric(kind)
    rows, Q = walk_corpus("dense")
    g = walk_gpu("dense")
    Q = Q[:4]
    ids, sc, cnt = g.search_metric(Q, 500, g_metric(metric))
    sparse = walk_sparse_rows("dense")
    cands = walk_candidates("dense", xo.candidate_count(500))
    assert cnt.tolist() == [500] * 4
    gap = 2.0 ** -21
    for i, q in enumerate(Q):
        qs = xo.Sparse(q)
        assert len(set(ids[i].tolist())) == 500
        want = np.array([xo.to_similarity(metric, xo.compute(metric, qs, sparse[int(n)])) for n in ids[i]], dtype=F)
        assert np.abs(sc[i].astype(np.float64) - want.astype(np.float64)).max() <= SIM_TOL
        assert np.all(sc[i][:-1] >= sc[i][1:])
        full = sorted(((nid, float(xo.to_similarity(metric, xo.compute(metric, qs, sparse[nid])))) for nid in cands[i]),
                      key=lambda t: -t[1])  # stable, descending
        assert len(full) == 800
        compared = 0
        for pos in range(500):
            s_here = full[pos][1]
            clear = (pos == 0 or full[pos - 1][1] - s_here >= gap) and (s_here - full[pos + 1][1] >= gap)
            if clear:
                compared += 1
                assert int(ids[i, pos]) == full[pos][0], (i, pos)
        cut = full[499][1]
        sure = {nid for nid, s in full if s - cut >= gap}
        maybe = {nid for nid, s in full if abs(s - cut) < gap}
        assert sure <= set(ids[i].tolist()) <= sure | maybe
        print(f"{metric} query {i}: {compared} of 500 positions compared id by id")


def test_stats_errors_and_the_empty_index():
    from neumann_amd import ExtendedDistanceMetric as M, GpuHnsw, NeumannGpuError, _capi
    g = walk_gpu("dense")
    _, Q = walk_corpus("dense")
    ids, sc, cnt, st = g.search_metric(Q[:3], 10, M.Euclidean, with_stats=True)
    assert st.sweep_kind == _capi.SWEEP_GRAPH and st.sweep == "graph"
    assert st.candidates_rescored == 20 and st.rows_scanned > 3 * 20
    ids, sc, cnt, st = g.search_metric(Q[:3], 500, M.Euclidean, with_stats=True)
    assert st.candidates_rescored == 800 and cnt.tolist() == [500, 500, 500]   # c is served as min(c, len)
    with pytest.raises(NeumannGpuError) as e:
        g.search_metric(Q[0], 0, M.Cosine)
    assert e.value.status == _capi.ERR_INVALID_TOP_K
    with pytest.raises(NeumannGpuError) as e:
        g.search_metric(Q[0], 5, M(9))
    assert e.value.status == _capi.ERR_CONFIGURATION
    with pytest.raises(NeumannGpuError) as e:
        g.search_metric_device(dev(Q[0]), 5, M(-1))
    assert e.value.status == _capi.ERR_CONFIGURATION
    with GpuHnsw(20) as empty:
        ids, sc, cnt = empty.search_metric(Q[:2], 3, M.Cosine)
        assert cnt.tolist() == [0, 0] and np.all(ids == np.uint64(2 ** 64 - 1)) and np.all(np.isneginf(sc))
        ids, sc, cnt = host(empty.search_metric_device(dev(Q[:2]), 3, M.Cosine))
        assert cnt.tolist() == [0, 0] and np.all(ids == np.uint64(2 ** 64 - 1)) and np.all(np.isneginf(sc))


def test_host_walk_gives_the_same_answer(monkeypatch):
    """NMN_HNSW_HOST_SEARCH=1: the walk on the host, the re-rank still on the device"""
    from neumann_amd import ExtendedDistanceMetric as M, GeometricConfig
    g = walk_gpu("sparse")
    _, Q = walk_corpus("sparse")
    for metric in (M.Composite(GeometricConfig.default()), M.WeightedJaccard):
        want = g.search_metric(Q, 10, metric, with_stats=True)
        monkeypatch.setenv("NMN_HNSW_HOST_SEARCH", "1")
        got = g.search_metric(Q, 10, metric, with_stats=True)
        monkeypatch.delenv("NMN_HNSW_HOST_SEARCH")
        assert_same_bits(got, want)
        assert got[3].rows_scanned > 0 and got[3].candidates_rescored == 20 == want[3].candidates_rescored
        assert got[3].sweep_launches == 0 and want[3].sweep_launches == 2


def test_the_large_k_sort_orders_as_the_rank_count(monkeypatch):
    """above 16 384 candidates the ordering goes through nmn_sortk.hip; NMN_XMETRIC_SORT_FROM lowers the threshold so that the
    two orderings can be held to each other on a small corpus: ties (the dense corpus under Jaccard: every score 1.0; duplicate
    rows under Cosine), a partly filled candidate block, top_k below and above the sort's tile"""
    from neumann_amd import ExtendedDistanceMetric as M
    for name in ("dense", "sparse"):
        g = walk_gpu(name)
        _, Q = walk_corpus(name)
        for metric in (M.Jaccard, M.Cosine, M.Manhattan):
            for top_k in (5, 10, 500):
                want = g.search_metric(Q, top_k, metric)
                monkeypatch.setenv("NMN_XMETRIC_SORT_FROM", "8")
                got = g.search_metric(Q, top_k, metric)
                got_dev = host(g.search_metric_device(dev(Q[:5]), top_k, metric))
                monkeypatch.delenv("NMN_XMETRIC_SORT_FROM")
                assert_same_bits(got, want)
                assert_same_bits(got_dev, (want[0][:5], want[1][:5], want[2][:5]))


def test_callers_sharing_a_stream_keep_their_own_candidates():
    """several threads on ONE stream (what stream=None means for every Python thread), different queries and shapes: growing the
    stream's candidate block, the walk, the re-rank and the ordering of a call are one unit, so each gets what it gets alone"""
    import threading
    import torch
    from neumann_amd import ExtendedDistanceMetric as M
    g = walk_gpu("sparse")
    _, Q = walk_corpus("sparse")
    jobs = [(Q[0:7], 5, M.Euclidean), (Q[7:8], 10, M.Cosine), (Q[8:33], 40, M.Manhattan), (Q[3:20], 1, M.WeightedJaccard)]
    want = [g.search_metric(q, k, m) for q, k, m in jobs]
    s = torch.cuda.Stream()
    qd = [dev(q) for q, _, _ in jobs]
    got = [[] for _ in jobs]
    errors = []

    def worker(i):
        try:
            for _ in range(25):
                got[i].append(g.search_metric_device(qd[i], jobs[i][1], jobs[i][2], stream=s))
        except Exception as e:  # noqa: BLE001
            errors.append(e)

    threads = [threading.Thread(target=worker, args=(i,)) for i in range(len(jobs))]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    s.synchronize()
    assert not errors, errors
    for i in range(len(jobs)):
        for res in got[i]:
            assert_same_bits(host(res), want[i])
