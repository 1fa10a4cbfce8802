"""nmn_hnsw_insert_embedding_tt / nmn_hnsw_tt_row (GpuHnsw.insert_embedding_tt / tt_row) against tests/_hnsw_ttnode_oracle.py: a
dense handle that holds EmbeddingStorage::TensorTrain nodes beside Dense and Sparse ones — levels, every neighbour list, the entry
point, ids and score BITS, through every search entry; TT queries through the TTN launches and through the host walk
(docs/hnsw.md §24)."""
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
from tests import _hnsw_tt_oracle as to
from tests import _hnsw_ttnode_oracle as tn

pytestmark = pytest.mark.gpu
F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "hnsw_ttnode_small.npz")
METRICS = [ho.COSINE, ho.EUCLIDEAN, ho.DOT_PRODUCT]
SV = mo.SparseVector
GEOM = {20: ([2, 2, 5], [1, 2, 2, 1]), 33: ([3, 11], [1, 3, 1])}


def bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


def assert_same(got, want):
    ig, sg, cg = got[:3]
    iw, sw, cw = want[:3]
    assert np.array_equal(cg, cw), (cg, cw)
    assert np.array_equal(ig, iw), np.argwhere(ig != iw)[:5]
    assert np.array_equal(bits(sg), bits(sw)), np.argwhere(bits(sg) != bits(sw))[:5]


def lib_tt(t):
    from neumann_amd import TTVector
    return TTVector(t.shape, t.ranks, t.cores)


def lib_tts(ts):
    return [lib_tt(t) for t in ts]


def dev(Q):
    import torch
    return torch.from_numpy(np.ascontiguousarray(np.atleast_2d(Q), dtype=F)).cuda()


def dev_cores(ts):
    import torch
    return torch.from_numpy(np.stack([t.flat() for t in ts])).cuda()


def host(res):
    import torch
    torch.cuda.synchronize()
    ids, sc, counts = res
    return ids.cpu().numpy().view(np.uint64), sc.cpu().numpy(), counts.cpu().numpy().astype(np.uint32)


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


def insert_items(g, items):
    """one call per item, in order: insert / insert_sparse / insert_embedding_tt"""
    for kind, x in items:
        if kind == "tt":
            g.insert_embedding_tt(lib_tt(x))
        elif kind == "sparse":
            g.insert_sparse(*g.sparse_from_dense(x.to_dense()))
        else:
            g.insert(np.asarray(x, dtype=F))


def assert_graph(g, o):
    assert len(g) == len(o)
    assert g.entry_point == o.entry_point and g.max_layer == o.max_layer
    assert g.levels().tolist() == o.levels
    for node in range(len(o)):
        for layer in range(o.levels[node] + 1):
            assert g.neighbors(node, layer).tolist() == o.neighbors[node][layer], (node, layer)


def tiled(want, reps, nq):
    """the answers of a tiled query set"""
    return tuple(np.concatenate([w] * reps)[:nq] for w in want)


def tt_entries(g, o, ts, k=10, ef=50, counts=(1, 2, 65, 257)):
    """TT queries `ts` (one rank vector) through search_tt and search_tt_device at several query counts (the set tiled), on the device"""
    want = tn.answers_tt(o, ts, k, ef)
    for nq in counts:
        reps = -(-nq // len(ts))
        qs = (ts * reps)[:nq]
        ids, sc, cnt, st = g.search_tt(lib_tts(qs), k, ef, with_stats=True)
        assert_same((ids, sc, cnt), tiled(want, reps, nq))
        assert st.sweep_launches == 3, "the device walk"
        assert_same(host(g.search_tt_device(ts[0].shape, ts[0].ranks, dev_cores(qs), k, ef)), tiled(want, reps, nq))
    return want


def dense_entries(g, o, Q, k=10, ef=50):
    """dense queries and their from_dense() forms through search, search_multi, search_device, search_sparse, search_sparse_multi"""
    want_d = mo.answers_dense(o, Q, k, ef)
    sqs = [SV.from_dense(q) for q in Q]
    want_s = mo.answers_sparse(o, sqs, k, ef)
    assert_same(g.search(Q, k, ef), want_d)
    assert_same(host(g.search_device(dev(Q), k, ef)), want_d)
    csr = g.sparse_from_dense(Q)
    assert_same(g.search_sparse(*csr, k, ef), want_s)
    ks = np.array([1 + (3 * i) % 12 for i in range(len(Q))], dtype=np.uint32)
    efs = np.array([0, 20, 64, 7] * (len(Q) // 4 + 1), dtype=np.uint32)[: len(Q)]
    kmax = int(ks.max())
    gd = g.search_multi(Q, ks, efs)
    gs = g.search_sparse_multi(*csr, ks, efs)
    for i in range(len(Q)):
        e = o.config.ef_search if efs[i] == 0 else int(efs[i])
        assert_same((gd[0][i:i + 1], gd[1][i:i + 1], gd[2][i:i + 1]), mo.padded([o.search_with_ef(Q[i], int(ks[i]), e)], kmax))
        assert_same((gs[0][i:i + 1], gs[1][i:i + 1], gs[2][i:i + 1]), mo.padded([o.search_sparse_with_ef(sqs[i], int(ks[i]), e)], kmax))
    return want_d


# ---- 1. the golden corpus, and what routing through insert_tt would answer -----------------------------------------------------------
def fixture_trains(z, prefix=""):
    ranks, off, cores = z[prefix + "ranks"], z[prefix + "core_off"], z[prefix + "cores"]
    out = []
    for q in range(len(ranks)):
        flat, cs, at = cores[int(off[q]):int(off[q + 1])], [], 0
        for k, n in enumerate(tn.GOLDEN_SHAPE):
            size = int(ranks[q][k]) * n * int(ranks[q][k + 1])
            cs.append(flat[at:at + size])
            at += size
        out.append(to.TTVector(tn.GOLDEN_SHAPE, ranks[q], cs))
    return out


def fixture_graph(z, name):
    idx = tn.HNSWTTNodeIndex(ho.HNSWConfig())
    idx.n = len(z["tt_mask"])
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


@pytest.mark.parametrize("name,metric", [("cosine", ho.COSINE), ("euclidean", ho.EUCLIDEAN), ("dot", ho.DOT_PRODUCT)])
def test_golden_corpus(name, metric):
    from neumann_amd import GpuHnsw, HNSWConfig
    z = np.load(GOLDEN)
    trains, tt_q = fixture_trains(z), fixture_trains(z, "q_")
    mask, Q = z["tt_mask"], z["dense_queries"]
    with GpuHnsw(20, HNSWConfig().with_distance_metric(metric)) as g, GpuHnsw(20, HNSWConfig().with_distance_metric(metric)) as twin:
        for t, m, row in zip(trains, mask, z["reconstructions"]):
            g.insert_embedding_tt(lib_tt(t)) if m else g.insert(row)
        assert_graph(g, fixture_graph(z, name))
        got_d = g.search(Q, 10, 50)
        assert_same(got_d, (z[f"{name}_ids"], z[f"{name}_scores"], z[f"{name}_counts"]))
        got_t = g.search_tt(lib_tts(tt_q), 10, 50)
        assert_same(got_t, (z[f"{name}_tt_ids"], z[f"{name}_tt_scores"], z[f"{name}_tt_counts"]))
        assert_same(host(g.search_tt_device(tn.GOLDEN_SHAPE, tn.GOLDEN_RANKS, dev_cores(tt_q), 10, 50)), got_t)
        assert g.memory_stats()["tt_count"] == int(mask.sum())
        # the same trains through insert_tt: Dense(reconstruction) nodes — the pinned counts say how far that is from a TT node
        twin.insert_tt(lib_tts(trains))
        assert g.levels().tolist() == twin.levels().tolist()
        lists = sum(1 for node in range(len(trains))
                    if any(g.neighbors(node, l).tolist() != twin.neighbors(node, l).tolist() for l in range(int(z[f"{name}_levels"][node]) + 1)))
        tw_d, tw_t = twin.search(Q, 10, 50), twin.search_tt(lib_tts(tt_q), 10, 50)
        got = (lists, tn.answers_differ(got_d, tw_d), tn.answers_differ(got_t, tw_t), int((got_t[0] != tw_t[0]).any(axis=1).sum()))
        print(f"{name}: lists, dense answers, TT answers, TT ids that differ from the insert_tt handle: {got}")
        assert got == tuple(int(z[f"{name}_{c}"]) for c in ("lists_differ", "dense_differ", "tt_differ", "tt_ids_differ"))
        assert got[2] >= 32 and (metric != ho.COSINE or (got[0] >= 1 and got[1] >= 32))
        assert g.hbm_bytes > twin.hbm_bytes


# ---- 2. Dense, Sparse and TT nodes interleaved: MIX and TTN together ----------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def interleaved(dim, n=90):
    """node i: i % 3 == 0 Dense, 1 Sparse (70 % zeros, doubled), 2 TT; clustered rows; 12 dense queries, 8 TT queries of one rank
    vector (another than the nodes': node rank != query rank)"""
    shape, ranks = GEOM[dim]
    rng = np.random.default_rng(dim * 7 + 1)
    rows = (rng.standard_normal((n, dim)) + 2.0 * rng.standard_normal((5, dim))[rng.integers(0, 5, n)]).astype(F)
    items = []
    for i in range(n):
        if i % 3 == 0:
            items.append(("dense", rows[i]))
        elif i % 3 == 1:
            items.append(("sparse", SV.from_dense(mo.sparsify(rng, rows[i:i + 1], 0.7)[0] * F(2.0))))
        else:
            items.append(("tt", to.random_tt(rng, shape, ranks)))
    Q = rng.standard_normal((12, dim)).astype(F)
    Q[8:][rng.random(Q[8:].shape) < 0.7] = 0.0
    qranks = [1] + [r + 1 for r in ranks[1:-1]] + [1]
    tq = [to.random_tt(rng, shape, qranks) for _ in range(8)]
    return items, Q, tq


@functools.lru_cache(maxsize=None)
def interleaved_oracle(dim, metric, n=90):
    return tn.build(interleaved(dim)[0][:n], o_cfg(metric))


@pytest.mark.parametrize("dim", [20, 33])
@pytest.mark.parametrize("metric", METRICS)
def test_interleaved_kinds_every_entry(dim, metric):
    from neumann_amd import GpuHnsw
    items, Q, tq = interleaved(dim)
    with GpuHnsw(dim, g_cfg(metric)) as g:
        insert_items(g, items[:60])
        o = interleaved_oracle(dim, metric, 60)
        assert_graph(g, o)
        assert_same(g.search_tt(lib_tts(tq), 10, 50), tn.answers_tt(o, tq, 10, 50))
        assert_same(g.search(Q, 10, 50), mo.answers_dense(o, Q, 10, 50))
        insert_items(g, items[60:])                       # after a further insert / insert_sparse / insert_embedding_tt
        o = interleaved_oracle(dim, metric)
        assert_graph(g, o)
        dense_entries(g, o, Q)
        tt_entries(g, o, tq)
        st = g.memory_stats()
        assert {k: st[k] for k in o.memory_stats()} == o.memory_stats()
        for node, (kind, x) in enumerate(items):
            assert np.array_equal(bits(g.get_vector(node)), bits(o.rows[node])), node
            row = g.tt_row(node)
            assert (row is None) == (kind != "tt")
            if row is not None:
                assert row.shape == x.shape and row.ranks == x.ranks
                assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(row.cores, x.cores))


def test_all_tt_handle_and_a_handle_of_one_tt_node():
    from neumann_amd import GpuHnsw
    shape, ranks = GEOM[20]
    rng = np.random.default_rng(0x7A1)
    ts = [to.random_tt(rng, shape, ranks) for _ in range(70)]
    tq = [to.random_tt(rng, shape, [1, 1, 2, 1]) for _ in range(6)]
    Q = rng.standard_normal((6, 20)).astype(F)
    for metric, n in ((ho.COSINE, 70), (ho.EUCLIDEAN, 70), (ho.COSINE, 1), (ho.DOT_PRODUCT, 1)):
        o = tn.build([("tt", t) for t in ts[:n]], o_cfg(metric))
        with GpuHnsw(20, g_cfg(metric)) as g:
            assert g.insert_embedding_tt(lib_tts(ts[:n])).tolist() == list(range(n))      # one call
            assert_graph(g, o)
            tt_entries(g, o, tq, counts=(1, 6))
            dense_entries(g, o, Q)
            assert g.memory_stats()["tt_count"] == n and g.memory_stats()["dense_count"] == 0
            assert g.memory_stats()["embedding_bytes"] == 4 * sum(t.flat().size for t in ts[:n])


# ---- 3. the trains a node may be ----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def train_zoo():
    """64 dimensions: nodes of 1, 2, 3 and 6 cores, modes of 1, ranks 1, 2, 8, 9 and the limit rank 32 — six shapes on one handle"""
    rng = np.random.default_rng(0x2009)
    geoms = [([64], [1, 1]), ([8, 8], [1, 2, 1]), ([8, 8], [1, 9, 1]), ([4, 4, 4], [1, 1, 1, 1]), ([4, 4, 4], [1, 8, 9, 1]),
             ([4, 4, 4], [1, 32, 32, 1]), ([2] * 6, [1, 2, 4, 3, 2, 2, 1]), ([1, 64], [1, 3, 1]), ([4, 1, 16], [1, 2, 2, 1]),
             ([4, 4, 4], [1, 2, 3, 1])]
    items = []
    for rep in range(4):
        for shape, ranks in geoms:
            items.append(("tt", to.random_tt(rng, shape, ranks, 0.5)))
        items.append(("dense", rng.standard_normal(64).astype(F)))
    queries = {"444": [to.random_tt(rng, [4, 4, 4], [1, 3, 2, 1], 0.5) for _ in range(4)],
               "444_wide": [to.random_tt(rng, [4, 4, 4], [1, 9, 8, 1], 0.5) for _ in range(2)],
               "88": [to.random_tt(rng, [8, 8], [1, 4, 1]) for _ in range(2)],
               "six": [to.random_tt(rng, [2] * 6, [1, 2, 2, 2, 2, 2, 1]) for _ in range(2)],
               "one": [to.random_tt(rng, [64], [1, 1]) for _ in range(2)],
               "ones": [to.random_tt(rng, [4, 1, 16], [1, 3, 1, 1]) for _ in range(2)]}
    return items, queries


@pytest.mark.parametrize("metric", [ho.COSINE, ho.EUCLIDEAN])
def test_node_trains_of_many_shapes_on_one_handle(metric):
    """a query meets nodes of its own shape (the Gram chain) and of five others (distance 1.0), with ranks unlike its own"""
    from neumann_amd import GpuHnsw
    items, queries = train_zoo()
    o = tn.build(items, o_cfg(metric))
    with GpuHnsw(64, g_cfg(metric)) as g:
        insert_items(g, items)
        assert_graph(g, o)
        assert g.tt_walk_limits()[:2] == (32, 0)
        for name, tq in queries.items():
            want = tt_entries(g, o, tq, k=12, ef=60, counts=(len(tq),))
            if name == "444":
                assert ((want[1] != 0) & np.isfinite(want[1])).any()
        rng = np.random.default_rng(3)
        dense_entries(g, o, rng.standard_normal((4, 64)).astype(F))


def test_a_node_above_the_tt_limits_sends_tt_queries_to_the_host_walk():
    """rank 33 is above nmn_tt_limits: the node is prepared by the host restatement, and from then on TT queries walk on the host
    with the same bits while the device entry refuses; dense queries go on riding the kernel"""
    from neumann_amd import GpuHnsw, _capi
    rng = np.random.default_rng(0x33)
    items = [("tt", to.random_tt(rng, [4, 4, 4], [1, 2, 3, 1], 0.5)) if i % 2 else ("dense", rng.standard_normal(64).astype(F))
             for i in range(40)]
    big = ("tt", to.random_tt(rng, [4, 4, 4], [1, 33, 2, 1], 0.2))
    tq = [to.random_tt(rng, [4, 4, 4], [1, 2, 2, 1], 0.5) for _ in range(4)]
    Q = rng.standard_normal((4, 64)).astype(F)
    with GpuHnsw(64, g_cfg(ho.COSINE)) as g:
        insert_items(g, items)
        o = tn.build(items, o_cfg(ho.COSINE))
        tt_entries(g, o, tq, counts=(4,))                                   # the kernel takes these nodes
        insert_items(g, [big])
        o.insert_embedding_tt(big[1])
        assert_graph(g, o)
        assert g.tt_walk_limits()[:2] == (33, 1)
        ids, sc, cnt, st = g.search_tt(lib_tts(tq), 10, 50, with_stats=True)
        assert_same((ids, sc, cnt), tn.answers_tt(o, tq, 10, 50))
        assert st.sweep_launches == 0, "the host walk"
        with pytest.raises(_capi.NeumannGpuError) as e:
            g.search_tt_device([4, 4, 4], [1, 2, 2, 1], dev_cores(tq), 10, 50)
        assert e.value.status == _capi.ERR_INVALID_ARGUMENT and "TensorTrain nodes" in str(e.value)
        assert_same(g.search(Q, 10, 50), mo.answers_dense(o, Q, 10, 50))
        assert np.array_equal(bits(g.get_vector(40)), bits(to.tt_reconstruct(big[1])))


def test_a_query_above_the_walks_lds_limit():
    """8192 dimensions leave the TT region under 8 K floats, less than nmn_tt_limits' max_storage: a train of ranks [1,20,11,1]
    (7552 core floats) walks on the device, one of ranks [1,21,11,1] (7912) is above the walk's limit — the host-buffer entry then
    walks on the host with the same bits, the device entry refuses.  (Both are within nmn_tt_limits, max_level included.)"""
    from neumann_amd import GpuHnsw, _capi
    rng = np.random.default_rng(0x8192)
    shape = [8, 32, 32]
    items = [("tt", to.random_tt(rng, shape, [1, 2, 2, 1], 0.05)) if i % 2 else ("dense", rng.standard_normal(8192).astype(F))
             for i in range(8)]
    fit = [to.random_tt(rng, shape, [1, 20, 11, 1], 0.05) for _ in range(2)]
    over = [to.random_tt(rng, shape, [1, 21, 11, 1], 0.05) for _ in range(2)]
    o = tn.build(items, o_cfg(ho.COSINE))
    with GpuHnsw(8192, g_cfg(ho.COSINE)) as g:
        insert_items(g, items)
        assert_graph(g, o)
        max_rank, above, floats = g.tt_walk_limits(50)
        assert (max_rank, above) == (2, 0)
        assert fit[0].flat().size + 2 * 2 * 20 <= floats < over[0].flat().size + 2 * 2 * 21 and over[0].flat().size <= 8192
        want = tn.answers_tt(o, fit, 5, 50)
        ids, sc, cnt, st = g.search_tt(lib_tts(fit), 5, 50, with_stats=True)
        assert_same((ids, sc, cnt), want)
        assert st.sweep_launches == 3
        assert_same(host(g.search_tt_device(shape, [1, 20, 11, 1], dev_cores(fit), 5, 50)), want)
        ids, sc, cnt, st = g.search_tt(lib_tts(over), 5, 50, with_stats=True)
        assert_same((ids, sc, cnt), tn.answers_tt(o, over, 5, 50))
        assert st.sweep_launches == 0, "the host walk"
        with pytest.raises(_capi.NeumannGpuError) as e:
            g.search_tt_device(shape, [1, 21, 11, 1], dev_cores(over), 5, 50)
        assert e.value.status == _capi.ERR_INVALID_ARGUMENT and "nmn_hnsw_tt_walk_limits" in str(e.value)


def single(x, shape=(2, 2, 5)):
    cores = [np.zeros(n, dtype=F) for n in shape]
    for c in cores:
        c[0] = 1.0
    cores[0][0] = x
    return to.TTVector(list(shape), [1] * (len(shape) + 1), cores)


@pytest.mark.parametrize("metric", [ho.COSINE, ho.DOT_PRODUCT])
def test_special_trains_in_one_call(metric):
    """the zero train and norms below, at and above 1e-10, as nodes and as queries of ONE call, beside ordinary trains"""
    from neumann_amd import GpuHnsw
    tiny = F(1e-10)
    rng = np.random.default_rng(0x5EC)
    shape, ranks = GEOM[20]
    zero = to.TTVector(shape, ranks, [np.zeros(4), np.zeros(8), np.zeros(10)])
    special = [zero, single(np.nextafter(tiny, F(0))), single(tiny), single(np.nextafter(tiny, F(1))), single(F(5e-11)),
               to.random_tt(rng, shape, ranks, 10.0 ** -3.6)]
    items = [("tt", t) for t in special]
    for i in range(40):
        items.append(("tt", to.random_tt(rng, shape, ranks)) if i % 2 else ("dense", rng.standard_normal(20).astype(F)))
    items += [("tt", t) for t in special]            # again, late: they meet T x T pruning with full lists
    o = tn.build(items, o_cfg(metric))
    one = [1, 1, 1, 1]
    tq = [to.TTVector(shape, one, [np.zeros(2), np.zeros(2), np.zeros(5)]), single(np.nextafter(tiny, F(0))), single(tiny),
          single(np.nextafter(tiny, F(1))), single(F(1.0)), to.random_tt(rng, shape, one), to.random_tt(rng, shape, one, 1e-4)]
    Q = np.stack([to.tt_reconstruct(single(F(1.0))), rng.standard_normal(20).astype(F), np.zeros(20, dtype=F)])
    with GpuHnsw(20, g_cfg(metric)) as g:
        insert_items(g, items)
        assert_graph(g, o)
        want = tt_entries(g, o, tq, counts=(len(tq),))
        assert (want[1][:2] == 0).all() and (want[1][2] != 0).any()      # a query norm below 1e-10: every distance is 1.0
        dense_entries(g, o, Q)


# ---- 4. around the walk -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", [ho.COSINE, ho.EUCLIDEAN])
def test_overflow_paths(metric):
    """(a) the LDS candidate heap set to 8 entries, (b) a results heap of 16 entries with ef 50 — both end in the spill launch"""
    from neumann_amd import GpuHnsw
    items, Q, tq = interleaved(20)
    o = interleaved_oracle(20, metric)
    want_t, want_d = tn.answers_tt(o, tq, 10, 50), mo.answers_dense(o, Q, 10, 50)
    with GpuHnsw(20, g_cfg(metric)) as g:
        insert_items(g, items)
        g.set_heap_capacity(candidates=8)
        ids, sc, cnt, st = g.search_tt(lib_tts(tq), 10, 50, with_stats=True)
        assert_same((ids, sc, cnt), want_t)
        assert st.fallback_queries > 0 and st.sweep_launches == 3
        assert_same(host(g.search_tt_device(tq[0].shape, tq[0].ranks, dev_cores(tq), 10, 50)), want_t)
        assert_same(g.search(Q, 10, 50), want_d)
        g.set_heap_capacity(results=16)
        ids, sc, cnt, st = g.search_tt(lib_tts(tq), 10, 50, with_stats=True)
        assert_same((ids, sc, cnt), want_t)
        assert st.fallback_queries == len(tq)
        assert_same(host(g.search_tt_device(tq[0].shape, tq[0].ranks, dev_cores(tq), 10, 50)), want_t)
        assert_same(g.search(Q, 10, 50), want_d)
        g.set_heap_capacity()
        ids, sc, cnt, st = g.search_tt(lib_tts(tq), 10, 50, with_stats=True)
        assert_same((ids, sc, cnt), want_t)
        assert st.fallback_queries == 0


def test_host_walk_in_child_process(tmp_path):
    """NMN_HNSW_HOST_SEARCH=1 in a fresh child process: the library's host walk — insert, dense, sparse and TT queries — is the twin"""
    items, Q, tq = interleaved(20)
    kinds = np.array([{"dense": 0, "sparse": 1, "tt": 2}[k] for k, _ in items])
    rows = np.stack([x if k == "dense" else x.to_dense() if k == "sparse" else np.zeros(20, dtype=F) for k, x in items])
    shape, ranks, off, cores = to.pack([x for k, x in items if k == "tt"])
    qshape, qranks, qoff, qcores = to.pack(tq)
    np.savez(tmp_path / "in.npz", kinds=kinds, rows=rows, shape=shape, ranks=ranks, off=off, cores=cores, qranks=qranks, qoff=qoff,
             qcores=qcores, Q=Q)
    code = (
        "import sys, numpy as np\n"
        f"sys.path.insert(0, {ROOT!r})\n"
        "from neumann_amd import GpuHnsw, HNSWConfig, TTVector\n"
        f"d = {str(tmp_path)!r}\n"
        "z = np.load(d + '/in.npz')\n"
        "def trains(shape, ranks, off, cores):\n"
        "    ts = []\n"
        "    for q in range(len(ranks)):\n"
        "        flat, cs, at = cores[int(off[q]):int(off[q + 1])], [], 0\n"
        "        for k in range(len(shape)):\n"
        "            n = int(ranks[q][k]) * int(shape[k]) * int(ranks[q][k + 1])\n"
        "            cs.append(flat[at:at + n])\n"
        "            at += n\n"
        "        ts.append(TTVector(shape, ranks[q], cs))\n"
        "    return ts\n"
        "nodes, tq = trains(z['shape'], z['ranks'], z['off'], z['cores']), trains(z['shape'], z['qranks'], z['qoff'], z['qcores'])\n"
        "out = {}\n"
        "for metric in (0, 1, 2):\n"
        "    with GpuHnsw(20, HNSWConfig.high_speed().with_distance_metric(metric)) as g:\n"
        "        t = 0\n"
        "        for kind, row in zip(z['kinds'], z['rows']):\n"
        "            if kind == 2:\n"
        "                g.insert_embedding_tt(nodes[t])\n"
        "                t += 1\n"
        "            elif kind == 1:\n"
        "                g.insert_sparse(*g.sparse_from_dense(row))\n"
        "            else:\n"
        "                g.insert(row)\n"
        "        ids, sc, cnt, st = g.search_tt(tq, 10, 50, with_stats=True)\n"
        "        assert st.sweep_launches == 0, st.sweep_launches\n"
        "        out[f'tt{metric}_ids'], out[f'tt{metric}_sc'], out[f'tt{metric}_cnt'] = ids, sc, cnt\n"
        "        out[f'd{metric}_ids'], out[f'd{metric}_sc'], out[f'd{metric}_cnt'] = g.search(z['Q'], 10, 50)\n"
        "        out[f's{metric}_ids'], out[f's{metric}_sc'], out[f's{metric}_cnt'] = g.search_sparse(*g.sparse_from_dense(z['Q']), 10, 50)\n"
        "        out[f'lv{metric}'] = g.levels()\n"
        "        out[f'l0{metric}'] = np.concatenate([g.neighbors(i, 0) for i in range(len(g))])\n"
        "np.savez(d + '/out.npz', **out)\n"
    )
    env = dict(os.environ, NMN_HNSW_HOST_SEARCH="1")
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    out = np.load(tmp_path / "out.npz")
    for metric in METRICS:
        o = interleaved_oracle(20, metric)
        assert out[f"lv{metric}"].tolist() == o.levels
        assert out[f"l0{metric}"].tolist() == [i for node in range(len(o)) for i in o.neighbors[node][0]]
        assert_same((out[f"tt{metric}_ids"], out[f"tt{metric}_sc"], out[f"tt{metric}_cnt"]), tn.answers_tt(o, tq, 10, 50))
        assert_same((out[f"d{metric}_ids"], out[f"d{metric}_sc"], out[f"d{metric}_cnt"]), mo.answers_dense(o, Q, 10, 50))
        assert_same((out[f"s{metric}_ids"], out[f"s{metric}_sc"], out[f"s{metric}_cnt"]),
                    mo.answers_sparse(o, [SV.from_dense(q) for q in Q], 10, 50))


def test_tt_dense_chain_and_insert_bulk_on_a_handle_with_tt_nodes():
    """§21's search_tt_dense decomposes the query and takes search_tt's path: it must score a TT node by its own rule; insert_bulk
    on such a handle walks on the host and builds the same graph"""
    from neumann_amd import GpuHnsw, TTConfig, tt_decompose
    items, Q, _ = interleaved(20)
    o = tn.build(items, o_cfg(ho.EUCLIDEAN))
    conf = TTConfig([2, 2, 5], max_rank=2, tolerance=1e-4)
    with GpuHnsw(20, g_cfg(ho.EUCLIDEAN)) as g:
        insert_items(g, items)
        dec = tt_decompose(Q[:4], conf)
        ts = [to.TTVector(t.shape, t.ranks, t.cores) for t in dec]
        assert_same(g.search_tt_dense(Q[:4], 10, conf), tn.answers_tt(o, ts, 10))
        extra = np.random.default_rng(8).standard_normal((6, 20)).astype(F)
        g.insert_bulk(extra)
        for r in extra:
            o.insert(r)
        assert_graph(g, o)
        assert g.bulk_stats()["walks"] == 0


def test_refusals_insert_and_write_nothing(tmp_path):
    from neumann_amd import GpuHnsw, _capi
    lib = _capi.load()
    shape, ranks = GEOM[20]
    rng = np.random.default_rng(0xBAD)
    good = [to.random_tt(rng, shape, ranks) for _ in range(2)]
    p = lambda a: C.c_void_p(a.ctypes.data)   # noqa: E731

    def call_insert(g, shape_, ranks_, off_, cores_, n):
        shape_, ranks_ = np.asarray(shape_, dtype=np.uint32), np.asarray(ranks_, dtype=np.uint32)
        off_, cores_ = np.asarray(off_, dtype=np.uint64), np.asarray(cores_, dtype=F)
        ids = np.full(n, 7, dtype=np.uint64)
        n0 = len(g)
        st = lib.nmn_hnsw_insert_embedding_tt(g._h, p(shape_), shape_.size, p(ranks_), p(off_), p(cores_), n, p(ids))
        assert (ids == 7).all() and len(g) == n0 and g.memory_stats()["tt_count"] == 0
        return st, lib.nmn_last_error().decode()

    sh, rk, off, cores = to.pack(good)
    with GpuHnsw(20, g_cfg(ho.COSINE), storage="quantized") as g:
        st, text = call_insert(g, sh, rk, off, cores, 2)
        assert st == _capi.ERR_CONFIGURATION and "dense handle only" in text
    with GpuHnsw(20, g_cfg(ho.COSINE), storage="binary") as g:
        st, text = call_insert(g, sh, rk, off, cores, 2)
        assert st == _capi.ERR_CONFIGURATION and "Binary" in text
    with GpuHnsw(20, g_cfg(ho.COSINE)) as g:
        bad = rk.copy()
        bad[1, 1] = 0
        st, text = call_insert(g, sh, bad, off, cores, 2)
        assert st == _capi.ERR_INVALID_ARGUMENT and "query 1" in text and ">= 1" in text
        bad_off = off.copy()
        bad_off[2] -= 1
        st, text = call_insert(g, sh, rk, bad_off, cores, 2)
        assert st == _capi.ERR_INVALID_ARGUMENT and "core_off" in text
        st, text = call_insert(g, [2, 2, 4], rk, [0, 20, 40], np.zeros(40), 2)       # well formed, another dimension
        assert st == _capi.ERR_DIMENSION_MISMATCH and "16" in text
        g.insert_embedding_tt(lib_tts(good))
        path = tmp_path / "tt.hnsw"
        with pytest.raises(_capi.NeumannGpuError) as e:
            g.save(path)
        assert e.value.status == _capi.ERR_CONFIGURATION and "TensorTrain" in str(e.value) and not os.path.exists(path)
    cfg = g_cfg(ho.COSINE)
    cfg.max_nodes = 3
    with GpuHnsw(20, cfg) as g:
        g.insert_embedding_tt(lib_tts(good))
        with pytest.raises(_capi.NeumannGpuError) as e:
            g.insert_embedding_tt(lib_tts(good))                                     # all or nothing
        assert e.value.status == _capi.ERR_CAPACITY and "HNSW index at capacity: 2 nodes (limit: 3)" in str(e.value) and len(g) == 2


def test_a_handle_without_tt_nodes_is_what_it_was(tmp_path):
    """no TT node: the same answers, the same statistics, the same file byte for byte — also after a refused insert_embedding_tt"""
    from neumann_amd import GpuHnsw, _capi
    rng = np.random.default_rng(0x0DD)
    rows = rng.standard_normal((80, 20)).astype(F)
    Q = rng.standard_normal((6, 20)).astype(F)
    tq = [to.random_tt(rng, *GEOM[20]) for _ in range(4)]
    o = ho.build(rows, o_cfg(ho.COSINE))
    files = []
    for attempt in (False, True):
        with GpuHnsw(20, g_cfg(ho.COSINE)) as g:
            g.insert(rows[:40])
            if attempt:
                with pytest.raises(_capi.NeumannGpuError):
                    g.insert_embedding_tt(lib_tt(to.random_tt(rng, [2, 2, 4], [1, 2, 2, 1])))
            g.insert(rows[40:])
            assert_graph(g, o)
            assert g.tt_walk_limits()[:2] == (0, 0) and g.tt_row(3) is None and g.memory_stats()["tt_count"] == 0
            assert_same(g.search(Q, 10, 50), ho.padded_answers(o, Q, 10, 50))
            ids, sc, cnt, st = g.search_tt(lib_tts(tq), 10, 50, with_stats=True)
            assert_same((ids, sc, cnt), to.answers_tt(o, tq, 10, 50))
            assert st.sweep_launches == 3
            path = tmp_path / f"plain{int(attempt)}.hnsw"
            g.save(path)
            files.append(open(path, "rb").read())
    assert files[0] == files[1]
    with GpuHnsw.load(tmp_path / "plain1.hnsw") as g2:
        assert_same(g2.search(Q, 10, 50), ho.padded_answers(o, Q, 10, 50))


def test_eight_threads_half_search_half_search_tt():
    items, Q, tq = interleaved(20)
    o = interleaved_oracle(20, ho.COSINE)
    want_tt = [tn.answers_tt(o, tq[2 * i:2 * i + 2], 10, 50) for i in range(4)]
    want_d = [mo.answers_dense(o, Q[2 * i:2 * i + 2], 10, 50) for i in range(4)]
    got, errors = {}, []
    from neumann_amd import GpuHnsw
    with GpuHnsw(20, g_cfg(ho.COSINE)) as g:
        insert_items(g, items)

        def work(i):
            try:
                for _ in range(5):
                    got[i] = g.search_tt(lib_tts(tq[2 * i:2 * i + 2]), 10, 50) if i < 4 else g.search(Q[2 * (i - 4):2 * (i - 4) + 2], 10, 50)
            except Exception as e:   # noqa: BLE001
                errors.append(e)
        threads = [threading.Thread(target=work, args=(i,)) for i in range(8)]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
    assert not errors, errors
    for i in range(4):
        assert_same(got[i], want_tt[i])
        assert_same(got[4 + i], want_d[i])
