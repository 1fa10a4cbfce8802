"""nmn_hnsw_insert_bulk (GpuHnsw.insert_bulk, docs/hnsw.md §19): the build walks batched on the GPU, commits on the host in order,
a device walk taken only when no list it read was assigned since its launch.  Held to the sequential graph of
tests/_hnsw_oracle.py list for list, to nmn_hnsw_insert byte for byte (the saved file: graph, rows, generator state), and to the
counts of tests/_hnsw_bulk_oracle.py exactly — accepted and conflicting walks are decided by which lists a walk reads, so equal
counts mean the kernel reads the lists the reference's algorithm reads."""
import functools
import json
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

from tests import _hnsw_bulk_oracle as bo
from tests import _hnsw_file as hf
from tests import _hnsw_oracle as ho

pytestmark = pytest.mark.gpu
F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
METRICS = [ho.COSINE, ho.EUCLIDEAN, ho.DOT_PRODUCT]
COUNTS = ("batches", "walks", "accepted", "conflicts", "host_nodes")


def g_cfg(o_cfg, **kw):
    from neumann_amd import HNSWConfig
    c = HNSWConfig(m=o_cfg.m, m0=o_cfg.m0, ef_construction=o_cfg.ef_construction, ef_search=o_cfg.ef_search,
                   distance_metric=o_cfg.distance_metric)
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def handle(o_cfg, dim, **kw):
    from neumann_amd import GpuHnsw
    return GpuHnsw(dim, g_cfg(o_cfg), **kw)


def assert_graph(g, o):
    assert len(g) == len(o)
    assert g.entry_point == o.entry_point and g.max_layer == o.max_layer
    assert g.levels().tolist() == o.levels
    for node in range(len(o)):
        for layer in range(o.levels[node] + 1):
            assert g.neighbors(node, layer).tolist() == o.neighbors[node][layer], (node, layer)
        assert g.neighbors(node, o.levels[node] + 1).size == 0


def assert_same_handles(a, b):
    assert len(a) == len(b) and a.entry_point == b.entry_point and a.max_layer == b.max_layer
    la, lb = a.levels().tolist(), b.levels().tolist()
    assert la == lb
    for node, lv in enumerate(la):
        for layer in range(lv + 1):
            assert a.neighbors(node, layer).tolist() == b.neighbors(node, layer).tolist(), (node, layer)


def saved(g, path):
    g.save(path)
    with open(path, "rb") as f:
        return f.read()


def check_stats(st):
    assert st["accepted"] + st["conflicts"] + st["overflowed"] == st["walks"], st


def assert_same(got, want):
    ig, sg, cg = got[:3]
    iw, sw, cw = want
    assert np.array_equal(cg, cw), (cg, cw)
    assert np.array_equal(ig, iw), np.argwhere(ig != iw)[:5]
    assert np.array_equal(np.ascontiguousarray(sg).view(np.uint32), np.ascontiguousarray(sw).view(np.uint32))


# ---- 1. the five corpora: the graph, the file, the counts -----------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(bo.CASES))
def test_bulk_graph_file_and_counts(name, tmp_path):
    rows, cfg, batch = bo.case_rows(name), bo.case_config(name), bo.CASES[name][6]
    want = bo.case_sequential(name)
    _, counts = bo.case_bulk(name)
    with handle(cfg, rows.shape[1]) as g, handle(cfg, rows.shape[1]) as s:
        g.set_bulk_policy(batch, 1)
        ids = g.insert_bulk(rows)
        assert ids.tolist() == list(range(len(rows)))
        st = g.bulk_stats()
        print(name, st)
        assert_graph(g, want)
        s.insert(rows)
        assert_same_handles(g, s)
        assert saved(g, tmp_path / "bulk.idx") == saved(s, tmp_path / "seq.idx")        # (the generator state is in the file)
        check_stats(st)
        assert {k: st[k] for k in COUNTS} == counts and st["overflowed"] == 0
        assert st["patched_lists"] > 0
        tr = g.bulk_trace()
        assert tr.shape == (st["batches"], 5) and int(tr[:, 0].sum()) == st["walks"] and int(tr[:, 1].sum()) == st["conflicts"]
        assert s.bulk_stats()["walks"] == 0 and s.bulk_stats()["host_nodes"] == 0      # nmn_hnsw_insert never counts


# ---- 2. ragged calls, both entries mixed; the adaptive policy ----------------------------------------------------------------------
@pytest.mark.parametrize("name", ["plain-default", "dup-eucl"])
def test_ragged_calls_and_adaptive_policy(name):
    rows, cfg = bo.case_rows(name), bo.case_config(name)
    want = bo.case_sequential(name)
    with handle(cfg, rows.shape[1]) as g:
        g.set_bulk_policy(8, 1)
        at = 0
        for i, b in enumerate([1, 1, 7, 100, 3, len(rows)]):
            part = rows[at:at + b]
            got = (g.insert if i % 2 else g.insert_bulk)(part)
            assert got.tolist() == list(range(at, at + len(part)))
            at += len(part)
        assert_graph(g, want)
        st = g.bulk_stats()
        check_stats(st)
        assert st["walks"] > 0 and st["host_nodes"] == 1 + 3                         # the empty index's first node; the 3-row call
    with handle(cfg, rows.shape[1]) as g:
        g.set_bulk_policy(0, 1)                                                        # adaptive: 8 at first, 4 .. 256
        g.insert_bulk(rows)
        assert_graph(g, want)
        st = g.bulk_stats()
        check_stats(st)
        sizes = g.bulk_trace()[:, 0]
        assert st["walks"] == len(rows) - 1 and sizes.max() <= 256 and sizes[0] <= 8
        # the sizes follow the rule: doubled after <= 1/4 redone, halved after >= 1/2, a cut or the call's end may shorten a batch
        b = 8
        for nb, redone in g.bulk_trace()[:, :2].tolist():
            assert nb <= b
            b = min(2 * b, 256) if 4 * redone <= nb else (max(b // 2, 4) if 2 * redone >= nb else b)
    with handle(cfg, rows.shape[1]) as g:                                              # the default min_nodes: below it, the host
        g.insert_bulk(rows)
        assert_graph(g, want)
        assert g.bulk_stats()["walks"] == 0 and g.bulk_stats()["host_nodes"] == len(rows)


# ---- 3. the entry point moves in the middle of a call -------------------------------------------------------------------------------
def test_entry_point_moves_mid_call(tmp_path):
    dim = 12
    rows = bo.make_rows("plain", 65, dim, 0xE17)
    cfg = ho.HNSWConfig()
    o = ho.HNSWIndex(cfg)                                                               # one level-0 node, the generator at its seed
    o.rows, o.mags = np.zeros((64, dim), dtype=F), np.zeros(64, dtype=F)
    o.rows[0], o.mags[0] = rows[0], ho.magnitude(rows[0])
    o.n, o.levels, o.neighbors, o.entry_point, o.max_layer, o.rng_seed = 1, [0], [[[]]], 0, 0, 42
    f = hf.HnswFile(dim=dim, quantized=False,
                    config=dict(m=cfg.m, m0=cfg.m0, ef_construction=cfg.ef_construction, ef_search=cfg.ef_search, ml=cfg.ml,
                                max_nodes=cfg.max_nodes, sparsity_threshold=0.5, distance_metric=cfg.distance_metric,
                                storage=hf.STORAGE_DENSE, reserved=0),
                    rng=42, entry_point=0, max_layer=0, levels=[0], nbr=[[[]]], rows=rows[:1].copy(),
                    mags=hf.chains_magnitude(rows[:1]))
    path = tmp_path / "one.idx"
    path.write_bytes(hf.write(f))
    counts = bo.bulk_insert(o, rows[1:], 64, 1)
    assert o.levels[1] == 7 and o.entry_point == 1 and counts["batches"] >= 2        # the first new node is cut off alone
    from neumann_amd import GpuHnsw
    with GpuHnsw.load(path) as g:
        g.set_bulk_policy(64, 1)
        g.insert_bulk(rows[1:])
        assert_graph(g, o)
        st = g.bulk_stats()
        assert {k: st[k] for k in COUNTS} == counts and st["overflowed"] == 0
        assert g.bulk_trace()[0, 0] == 1
        with GpuHnsw.load(path) as s:
            s.insert(rows[1:])
            assert saved(g, tmp_path / "a.idx") == saved(s, tmp_path / "b.idx")


# ---- 4. overflow ----------------------------------------------------------------------------------------------------------------------
def test_overflowed_walks_and_small_result_heaps():
    name = "plain-cos"
    rows, cfg = bo.case_rows(name), bo.case_config(name)
    want = bo.case_sequential(name)
    with handle(cfg, rows.shape[1]) as g:
        g.set_bulk_policy(8, 1)
        g.set_heap_capacity(candidates=8)                                              # the walks of this corpus fill it
        g.insert_bulk(rows)
        assert_graph(g, want)
        st = g.bulk_stats()
        check_stats(st)
        assert st["overflowed"] > 0 and st["walks"] == len(rows) - 1
    with handle(cfg, rows.shape[1]) as g:
        g.set_bulk_policy(8, 1)
        g.set_heap_capacity(results=cfg.ef_construction)                               # below ef_construction + 1: never launched
        g.insert_bulk(rows)
        assert_graph(g, want)
        st = g.bulk_stats()
        assert st["walks"] == 0 and st["batches"] == 0 and st["host_nodes"] == len(rows)


# ---- 5. dimensions: tail chunks, one-pass and multi-pass rows; a zero row under Cosine ------------------------------------------
@functools.lru_cache(maxsize=None)
def dim_case(dim, metric):
    rows = bo.make_rows("plain", 200, dim, 0xD1 + dim)
    rows[50] = 0.0
    rows[120] = 0.0
    cfg = ho.HNSWConfig(m=8, ef_construction=16, distance_metric=metric)
    return rows, cfg, ho.build(rows, cfg)


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("dim", [3, 8, 13, 33, 130])
def test_dimensions_and_zero_rows(dim, metric):
    rows, cfg, want = dim_case(dim, metric)
    with handle(cfg, dim) as g:
        g.set_bulk_policy(8, 1)
        g.insert_bulk(rows)
        assert_graph(g, want)
        st = g.bulk_stats()
        check_stats(st)
        assert st["walks"] == 199 and st["overflowed"] == 0 and st["accepted"] > 0


# ---- 6. handles the device does not walk for; errors ----------------------------------------------------------------------------------
def test_ineligible_handles_take_the_host_path():
    from neumann_amd import GpuHnsw
    name = "plain-default"
    rows, cfg = bo.case_rows(name)[:200], bo.case_config(name)
    for storage in ("quantized", "binary"):
        with GpuHnsw(rows.shape[1], g_cfg(cfg), storage=storage) as a, GpuHnsw(rows.shape[1], g_cfg(cfg), storage=storage) as b:
            a.set_bulk_policy(8, 1)
            a.insert_bulk(rows)
            b.insert(rows)
            assert_same_handles(a, b)
            st = a.bulk_stats()
            assert st["walks"] == 0 and st["host_nodes"] == len(rows)
    sparse = np.zeros((1, rows.shape[1]), dtype=F)
    sparse[0, 3] = 1.5
    with handle(cfg, rows.shape[1]) as a, handle(cfg, rows.shape[1]) as b:             # a dense handle holding one Sparse node
        for g in (a, b):
            g.insert(rows[:20])
            g.insert_auto(sparse)
        assert a.sparse_row(20) is not None
        a.set_bulk_policy(8, 1)
        a.insert_bulk(rows[20:])
        b.insert(rows[20:])
        assert_same_handles(a, b)
        st = a.bulk_stats()
        assert st["walks"] == 0 and st["host_nodes"] == len(rows) - 20


def test_errors_are_those_of_insert():
    from neumann_amd import GpuHnsw, HNSWConfig, NeumannGpuError, _capi
    with GpuHnsw(4, HNSWConfig(max_nodes=3)) as g:
        g.set_bulk_policy(2, 1)
        g.insert_bulk(np.eye(4, dtype=F)[:2])
        with pytest.raises(NeumannGpuError, match=r"HNSW index at capacity: 2 nodes \(limit: 3\)") as e:
            g.insert_bulk(np.ones((2, 4), F))                                           # all or nothing
        assert e.value.status == _capi.ERR_CAPACITY and len(g) == 2
        g.insert_bulk(np.eye(4, dtype=F)[2:3])
        with pytest.raises(NeumannGpuError, match=r"HNSW index at capacity: 3 nodes \(limit: 3\)") as e:
            g.insert_bulk(np.ones((1, 4), F))
        assert e.value.status == _capi.ERR_CAPACITY and len(g) == 3
        with pytest.raises(NeumannGpuError) as e:
            g.insert_bulk(np.ones((1, 5), F))
        assert e.value.status == _capi.ERR_DIMENSION_MISMATCH
        assert g.insert_bulk(np.zeros((0, 4), F)).size == 0
        assert g._lib.nmn_hnsw_insert_bulk(g._h, None, 1, None) == _capi.ERR_INVALID_ARGUMENT
        assert g._lib.nmn_hnsw_insert(g._h, None, 1, None) == _capi.ERR_INVALID_ARGUMENT
        with pytest.raises(NeumannGpuError) as e:
            g.set_bulk_policy(5000, 0)
        assert e.value.status == _capi.ERR_INVALID_ARGUMENT


# ---- 7. searches after a bulk build; a bulk build under searching threads ---------------------------------------------------------
def test_searches_after_a_bulk_build_and_concurrent_searches():
    import torch
    name = "plain-cos"
    rows, cfg = bo.case_rows(name), bo.case_config(name)
    want = bo.case_sequential(name)
    rng = np.random.default_rng(77)
    Q = rng.standard_normal((16, rows.shape[1])).astype(F)
    Q[:4] = rows[rng.integers(0, len(rows), 4)]
    half = len(rows) // 2
    with handle(cfg, rows.shape[1]) as g:
        g.set_bulk_policy(8, 1)
        g.insert_bulk(rows[:half])
        stop, errs = threading.Event(), []

        def work(t):
            try:
                while not stop.is_set():
                    ids, _, cnt = g.search(Q[2 * t:2 * t + 2], 10)
                    assert cnt.tolist() == [10] * 2 and int(ids.max()) < len(rows)
            except Exception as e:  # noqa: BLE001
                errs.append(e)

        th = [threading.Thread(target=work, args=(t,)) for t in range(8)]
        [t.start() for t in th]
        try:
            for at in range(half, len(rows), 150):
                g.insert_bulk(rows[at:at + 150])
        finally:
            stop.set()
            [t.join() for t in th]
        assert not errs, errs
        assert_graph(g, want)
        check_stats(g.bulk_stats())
        for k, ef in ((50, None), (7, 300)):
            assert_same(g.search(Q, k, ef), ho.padded_answers(want, Q, k, ef))
        ks = np.asarray([1 + 3 * (i % 4) for i in range(len(Q))], dtype=np.uint32)
        got = g.search_multi(Q, ks)
        for i, k in enumerate(ks.tolist()):
            wi, ws, wc = ho.padded_answers(want, Q[i], k)
            assert got[2][i] == wc[0] and got[0][i, :k].tolist() == wi[0].tolist()
            assert got[1][i, :k].view(np.uint32).tolist() == ws[0].view(np.uint32).tolist()
        qd = torch.from_numpy(Q).cuda()
        out = g.search_device(qd, 10)
        torch.cuda.synchronize()
        w10 = ho.padded_answers(want, Q, 10)
        assert_same((out[0].cpu().numpy().view(np.uint64), out[1].cpu().numpy(), out[2].cpu().numpy().astype(np.uint32)), w10)
        ids, sc, cnt, stt = g.search(Q[:4], 10, 1100, with_stats=True)                 # results heap beyond LDS: the spill launch
        assert_same((ids, sc, cnt), ho.padded_answers(want, Q[:4], 10, 1100))
        assert stt.fallback_queries == 4
        g.set_heap_capacity(candidates=8)                                              # candidate heap overflow
        ids, sc, cnt, stt = g.search(Q, 10, with_stats=True)
        assert_same((ids, sc, cnt), w10)
        assert stt.fallback_queries > 0


# ---- 8. NMN_HNSW_BULK_BUILD=1 routes the engine's build through the bulk path --------------------------------------------------------
def test_env_routes_the_engines_build(tmp_path):
    n, dim = 600, 16                                                                    # (below the default min_nodes: host walks)
    rows = bo.make_rows("plain", n, dim, 0xE8)
    np.save(tmp_path / "rows.npy", rows)
    code = (
        "import sys, json, numpy as np\n"
        f"sys.path.insert(0, {ROOT!r})\n"
        "from neumann_amd import engine, HNSWConfig\n"
        f"d = {str(tmp_path)!r}\n"
        "rows = np.load(d + '/rows.npy')\n"
        "eng = engine.VectorEngine()\n"
        "for i, r in enumerate(rows):\n"
        "    eng.store_embedding(f'key{i:05d}', r)\n"
        "index, keys = eng.build_hnsw_index(HNSWConfig.high_speed())\n"
        "g = index.gpu()\n"
        "g.save(d + '/child.idx')\n"
        "json.dump(dict(keys=keys, stats=g.bulk_stats()), open(d + '/child.json', 'w'))\n"
    )
    env = dict(os.environ, NMN_HNSW_BULK_BUILD="1")
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    with open(tmp_path / "child.json") as f:
        child = json.load(f)
    st = child["stats"]
    check_stats(st)
    assert st["host_nodes"] == n and st["walks"] == 0                                  # the bulk entry ran: nmn_hnsw_insert counts nothing
    order = [int(k[3:]) for k in child["keys"]]
    from neumann_amd import GpuHnsw, HNSWConfig
    assert "NMN_HNSW_BULK_BUILD" not in os.environ
    with GpuHnsw(dim, HNSWConfig.high_speed()) as s:
        s.insert(rows[order])
        assert s.bulk_stats()["walks"] == 0
        assert saved(s, tmp_path / "here.idx") == (tmp_path / "child.idx").read_bytes()
