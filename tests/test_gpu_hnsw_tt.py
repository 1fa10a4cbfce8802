"""nmn_tt_reconstruct / nmn_tt_norm and nmn_hnsw_search_tt / _search_tt_device / _insert_tt (neumann_amd.tt, GpuHnsw.search_tt /
search_tt_device / insert_tt) against tests/_hnsw_tt_oracle.py: reconstructions and norms, ids and score BITS (docs/hnsw.md §17)."""
import functools
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

from tests import _hnsw_mixed_oracle as mo
from tests import _hnsw_oracle as ho
from tests import _hnsw_q8_oracle as qo
from tests import _hnsw_tt_oracle as to

pytestmark = pytest.mark.gpu
F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
METRICS = [ho.COSINE, ho.EUCLIDEAN, ho.DOT_PRODUCT]
SHAPE, RANKS, DIM = [2, 2, 5], [1, 2, 2, 1], 20


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


def host(res):
    import torch
    torch.cuda.synchronize()
    ids, sc, counts = res
    return ids.cpu().numpy().view(np.uint64), sc.cpu().numpy(), counts.cpu().numpy().astype(np.uint32)


def dev_cores(ts):
    import torch
    return torch.from_numpy(np.stack([t.flat() for t in ts])).cuda()


def o_cfg(metric):
    return ho.HNSWConfig.high_speed().with_distance_metric(metric)


def g_cfg(metric):
    from neumann_amd import HNSWConfig
    return HNSWConfig.high_speed().with_distance_metric(metric)


# ---- 1. the preparation alone --------------------------------------------------------------------------------------------------------
def assert_prepared(ts):
    from neumann_amd import tt_norm, tt_reconstruct
    want_r = np.stack([to.tt_reconstruct(t) for t in ts])
    want_n = np.asarray([to.tt_norm(t) for t in ts], dtype=F)
    got_r, got_n = tt_reconstruct(lib_tts(ts)), tt_norm(lib_tts(ts))
    assert np.array_equal(bits(got_r), bits(want_r)), np.argwhere(bits(got_r) != bits(want_r))[:5]
    assert np.array_equal(bits(got_n), bits(want_n)), np.argwhere(bits(got_n) != bits(want_n))[:5]


PREP = {
    "dim1_one_core": ([1], [1, 1]),
    "dim5_mode_of_1": ([1, 5], [1, 3, 1]),
    "dim7_one_core": ([7], [1, 1]),
    "dim20_three_cores": ([2, 2, 5], [1, 2, 2, 1]),
    "dim33_two_cores": ([3, 11], [1, 2, 1]),
    "dim64_six_cores": ([2] * 6, [1, 2, 4, 3, 2, 2, 1]),
    "dim768": ([8, 8, 12], [1, 8, 8, 1]),
    "all_one_ranks": ([4, 4, 4], [1, 1, 1, 1]),
    "non_monotone": ([3, 4, 5], [1, 4, 2, 1]),
    "mode_of_1_inside": ([3, 1, 5], [1, 4, 2, 1]),
    "ranks_at_the_limit": ([2, 3, 2], [1, 32, 32, 1]),
}


@pytest.mark.parametrize("case", sorted(PREP))
def test_preparation_bit_for_bit(case):
    shape, ranks = PREP[case]
    rng = np.random.default_rng(sum(map(ord, case)))
    assert_prepared([to.random_tt(rng, shape, ranks) for _ in range(3)])


def test_preparation_at_and_beyond_the_lds_limits():
    """storage exactly 8192 floats (the kernel), 9216 (the host restatement), a rank of 33 and a level above the limit — in ONE call
    where the shape allows, so the launch skips what the host prepares"""
    from neumann_amd import tt
    max_cores, max_rank, max_storage, max_level = tt.limits()
    assert (max_cores, max_rank, max_storage) == (8, 32, 8192) and max_level >= 2048
    rng = np.random.default_rng(81)
    at, beyond = to.random_tt(rng, [8, 1016], [1, 8, 1], 0.05), to.random_tt(rng, [8, 1016], [1, 9, 1], 0.05)
    assert at.flat().size == max_storage and beyond.flat().size > max_storage
    assert_prepared([at, beyond, at])
    assert_prepared([to.random_tt(rng, [2, 3, 2], [1, 33, 33, 1], 0.2), to.random_tt(rng, [2, 3, 2], [1, 32, 32, 1], 0.2)])
    wide = to.random_tt(rng, [128, 2], [1, 32, 1], 0.2)      # level 1 holds 128 x 32 floats
    assert 128 * 32 > max_level
    assert_prepared([wide])


def test_preparation_ranks_per_query_and_counts_past_the_grid():
    rng = np.random.default_rng(5)
    mixed = [to.random_tt(rng, [4, 4, 8], r) for r in ([1, 3, 3, 1], [1, 1, 1, 1], [1, 4, 2, 1], [1, 2, 4, 1], [1, 4, 4, 1])]
    assert_prepared(mixed)
    many = [to.random_tt(rng, SHAPE, RANKS if i % 3 else [1, 1, 2, 1]) for i in range(257)]
    for nq in (1, 2, 65, 257):
        assert_prepared(many[:nq])


# ---- 2. every kind of handle, through search_tt and search_tt_device -----------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def corpus(n=200):
    rng = np.random.default_rng(0x7751)
    rows = (rng.standard_normal((n, DIM)) + 2.0 * rng.standard_normal((6, DIM))[rng.integers(0, 6, n)]).astype(F)
    mask = np.arange(n) % 2 == 1
    rows[mask] = mo.sparsify(rng, rows[mask], 0.7) * F(2.0)
    rows[40] = 0.0     # a Dense node of magnitude 0
    rows[41] = 0.0     # ... and a Sparse one (in the mixed handles)
    return rows, mask


@functools.lru_cache(maxsize=None)
def trains():
    """12 Gaussian trains of ranks [1,2,2,1], three of other ranks (so one call carries ranks that differ) and one scaled by 30"""
    rng = np.random.default_rng(0x7752)
    ts = [to.random_tt(rng, SHAPE, RANKS) for _ in range(12)]
    ts += [to.random_tt(rng, SHAPE, [1, 1, 2, 1]), to.random_tt(rng, SHAPE, [1, 2, 1, 1]), to.random_tt(rng, SHAPE, [1, 1, 1, 1]),
           to.random_tt(rng, SHAPE, [1, 2, 2, 1], 30.0)]
    return ts


def uniform_trains():
    return [t for t in trains() if t.ranks == RANKS]


@functools.lru_cache(maxsize=None)
def oracle(kind, metric):
    rows, mask = corpus()
    if kind == "dense":
        return ho.build(rows, o_cfg(metric))
    if kind == "q8":
        return qo.build(rows, o_cfg(metric))
    if kind == "mixed":
        return mo.build_mixed(rows, mask, o_cfg(metric))
    if kind == "sparse":
        return mo.build_mixed(rows, np.ones(len(rows), dtype=bool), o_cfg(metric))
    raise KeyError(kind)


def gpu_index(kind, metric):
    from neumann_amd import GpuHnsw
    rows, mask = corpus()
    g = GpuHnsw(DIM, g_cfg(metric), storage="quantized" if kind == "q8" else None)
    if kind in ("dense", "q8"):
        g.insert(rows)
    else:
        m = mask if kind == "mixed" else np.ones(len(rows), dtype=bool)
        for i in range(len(rows)):
            g.insert_sparse(*g.sparse_from_dense(rows[i])) if m[i] else g.insert(rows[i])
    return g


KINDS = [("dense", ho.COSINE), ("dense", ho.EUCLIDEAN), ("dense", ho.DOT_PRODUCT), ("q8", ho.COSINE), ("q8", ho.EUCLIDEAN),
         ("mixed", ho.COSINE), ("mixed", ho.EUCLIDEAN), ("mixed", ho.DOT_PRODUCT), ("sparse", ho.COSINE)]


@pytest.mark.parametrize("kind,metric", KINDS)
def test_handle_kinds(kind, metric):
    o = oracle(kind, metric)
    ts = trains()
    want = to.answers_tt(o, ts, 10, 50)
    with gpu_index(kind, metric) as g:
        ids, sc, cnt, st = g.search_tt(lib_tts(ts), 10, 50, with_stats=True)
        assert_same((ids, sc, cnt), want)
        assert st.sweep == "graph" and st.rows_scanned > 0 and st.fallback_queries == 0 and st.sweep_launches == 3
        assert_same(g.search_tt(lib_tts(ts), 3), to.answers_tt(o, ts, 3))                          # ef None: ef_search
        assert_same(g.search_tt(lib_tt(ts[0]), 7, 11), to.answers_tt(o, ts[:1], 7, 11))            # nq = 1
        assert_same(g.search_tt(lib_tts(ts), 300, 20), to.answers_tt(o, ts, 300, 20))              # k > ef, k > n
        us = uniform_trains()
        assert_same(host(g.search_tt_device(SHAPE, RANKS, dev_cores(us), 10, 50)), to.answers_tt(o, us, 10, 50))
        if metric != ho.COSINE and kind == "dense":   # nothing in common with `search` of the reconstruction
            dids, dsc, _ = g.search(np.stack([to.tt_reconstruct(t) for t in ts]), 10, 50)
            assert ((dids != ids) | (bits(dsc) != bits(sc))).any(axis=1).all()


def test_empty_index_and_one_node():
    from neumann_amd import GpuHnsw
    ts = uniform_trains()[:3]
    for metric in (ho.COSINE, ho.EUCLIDEAN):
        o = ho.HNSWIndex(o_cfg(metric))
        with GpuHnsw(DIM, g_cfg(metric)) as g:
            ids, sc, cnt, st = g.search_tt(lib_tts(ts), 4, with_stats=True)
            assert_same((ids, sc, cnt), to.answers_tt(o, ts, 4))
            assert cnt.tolist() == [0, 0, 0] and st.sweep == "none"
            assert_same(host(g.search_tt_device(SHAPE, RANKS, dev_cores(ts), 4)), to.answers_tt(o, ts, 4))
            row = corpus()[0][3]
            o.insert(row)
            g.insert(row)
            assert_same(g.search_tt(lib_tts(ts), 4), to.answers_tt(o, ts, 4))
            assert_same(host(g.search_tt_device(SHAPE, RANKS, dev_cores(ts), 4)), to.answers_tt(o, ts, 4))


def test_host_walk_in_child_process(tmp_path):
    """NMN_HNSW_HOST_SEARCH=1 in a fresh child process: host preparation and host walk, the same bits"""
    rows, mask = corpus()
    ts = trains()
    shape, ranks, off, cores = to.pack(ts)
    np.savez(tmp_path / "in.npz", rows=rows, mask=mask, shape=shape, ranks=ranks, off=off, cores=cores)
    code = (
        "import sys, numpy as np\n"
        f"sys.path.insert(0, {ROOT!r})\n"
        "from neumann_amd import GpuHnsw, HNSWConfig, TTVector, tt_norm, tt_reconstruct\n"
        f"d = {str(tmp_path)!r}\n"
        "z = np.load(d + '/in.npz')\n"
        "rows, mask, shape, ranks, off, cores = (z[k] for k in ('rows', 'mask', 'shape', 'ranks', 'off', 'cores'))\n"
        "ts = []\n"
        "for q in range(len(ranks)):\n"
        "    flat, cs, at = cores[int(off[q]):int(off[q + 1])], [], 0\n"
        "    for k in range(len(shape)):\n"
        "        n = int(ranks[q][k]) * int(shape[k]) * int(ranks[q][k + 1])\n"
        "        cs.append(flat[at:at + n])\n"
        "        at += n\n"
        "    ts.append(TTVector(shape, ranks[q], cs))\n"
        "out = {'recon': tt_reconstruct(ts), 'norms': tt_norm(ts)}\n"
        "for kind, metric in (('dense', 0), ('dense', 1), ('dense', 2), ('q8', 0), ('mixed', 0), ('mixed', 1), ('sparse', 0),\n"
        "                     ('empty', 1), ('one', 1)):\n"
        "    with GpuHnsw(rows.shape[1], HNSWConfig.high_speed().with_distance_metric(metric),\n"
        "                 storage='quantized' if kind == 'q8' else None) as g:\n"
        "        for i in range({'empty': 0, 'one': 1}.get(kind, len(rows))):\n"
        "            as_sparse = kind == 'sparse' or (kind == 'mixed' and mask[i])\n"
        "            g.insert_sparse(*g.sparse_from_dense(rows[i])) if as_sparse else g.insert(rows[i])\n"
        "        ids, sc, cnt, st = g.search_tt(ts, 10, 50, with_stats=True)\n"
        "        assert st.sweep_launches == 0, st.sweep_launches\n"
        "        out[f'{kind}{metric}_ids'], out[f'{kind}{metric}_sc'], out[f'{kind}{metric}_cnt'] = ids, sc, cnt\n"
        "np.savez(d + '/out.npz', **out)\n"
    )
    env = dict(os.environ, NMN_HNSW_HOST_SEARCH="1")
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    out = np.load(tmp_path / "out.npz")
    assert np.array_equal(bits(out["recon"]), bits(np.stack([to.tt_reconstruct(t) for t in ts])))
    assert np.array_equal(bits(out["norms"]), bits(np.asarray([to.tt_norm(t) for t in ts], dtype=F)))
    for kind, metric in (("dense", 0), ("dense", 1), ("dense", 2), ("q8", 0), ("mixed", 0), ("mixed", 1), ("sparse", 0), ("empty", 1),
                         ("one", 1)):
        if kind in ("empty", "one"):
            o = ho.HNSWIndex(o_cfg(metric))
            for r in rows[:1 if kind == "one" else 0]:
                o.insert(r)
        else:
            o = oracle(kind, metric)
        want = to.answers_tt(o, ts, 10, 50)
        assert_same((out[f"{kind}{metric}_ids"], out[f"{kind}{metric}_sc"], out[f"{kind}{metric}_cnt"]), want)


# ---- 3. around the walk ---------------------------------------------------------------------------------------------------------------
def special_trains():
    """the zero train; norms below, at and above 1e-10; a NaN core element; a mode-of-1 style train with all-one ranks"""
    one = [1, 1, 1, 1]

    def single(x):   # reconstruction = x at element 0, zeros elsewhere: the norm is sqrt(x * x)
        return to.TTVector(SHAPE, one, [np.array([x, 0], dtype=F), np.array([1, 0], dtype=F), np.array([1, 0, 0, 0, 0], dtype=F)])

    tiny = F(1e-10)
    rng = np.random.default_rng(9)
    nan = to.random_tt(rng, SHAPE, RANKS)
    nan.cores[1][1, 0, 1] = np.nan
    ts = [to.TTVector(SHAPE, one, [np.zeros(2, dtype=F), np.zeros(2, dtype=F), np.zeros(5, dtype=F)]),
          single(np.nextafter(tiny, F(0))), single(tiny), single(np.nextafter(tiny, F(1))), nan, to.random_tt(rng, SHAPE, one),
          to.random_tt(rng, SHAPE, RANKS)]
    norms = [to.tt_norm(t) for t in ts]
    assert norms[0] == 0 and norms[1] < tiny and bits(norms[2]) == bits(tiny) and norms[3] > tiny and np.isnan(norms[4])
    return ts


@pytest.mark.parametrize("kind,metric", [("dense", ho.COSINE), ("dense", ho.EUCLIDEAN), ("q8", ho.COSINE), ("mixed", ho.DOT_PRODUCT)])
def test_special_trains_in_one_call(kind, metric):
    o = oracle(kind, metric)
    ts = special_trains()
    want = to.answers_tt(o, ts, 10, 50)
    assert (want[1][:2] == 0).all() and (want[1][2] != 0).any()   # below 1e-10 every distance is 1.0; at it the arithmetic runs
    with gpu_index(kind, metric) as g:
        assert_same(g.search_tt(lib_tts(ts), 10, 50), want)
        assert_prepared(ts)


def test_after_insert_and_after_save_load(tmp_path):
    from neumann_amd import GpuHnsw
    rows, _ = corpus()
    ts = trains()
    for metric in (ho.COSINE, ho.DOT_PRODUCT):
        o = ho.build(rows[:150], o_cfg(metric))
        with GpuHnsw(DIM, g_cfg(metric)) as g:
            g.insert(rows[:150])
            assert_same(g.search_tt(lib_tts(ts), 10, 50), to.answers_tt(o, ts, 10, 50))
            for r in rows[150:]:
                o.insert(r)
            g.insert(rows[150:])
            want = to.answers_tt(o, ts, 10, 50)
            assert_same(g.search_tt(lib_tts(ts), 10, 50), want)
            path = tmp_path / f"tt_{metric}.hnsw"
            g.save(path)
        with GpuHnsw.load(path) as g2:
            assert_same(g2.search_tt(lib_tts(ts), 10, 50), want)
            us = uniform_trains()
            assert_same(host(g2.search_tt_device(SHAPE, RANKS, dev_cores(us), 10, 50)), to.answers_tt(o, us, 10, 50))


@pytest.mark.parametrize("kind,metric", [("dense", ho.EUCLIDEAN), ("q8", ho.COSINE), ("mixed", ho.COSINE)])
def test_overflow_paths(kind, metric):
    """(a) the LDS candidate heap set to 8 entries, (b) a results heap of 16 entries with ef 50 — both end in the spill launch"""
    o = oracle(kind, metric)
    ts, us = trains(), uniform_trains()
    want, want_u = to.answers_tt(o, ts, 10, 50), to.answers_tt(o, us, 10, 50)
    with gpu_index(kind, metric) as g:
        g.set_heap_capacity(candidates=8)
        ids, sc, cnt, st = g.search_tt(lib_tts(ts), 10, 50, with_stats=True)
        assert_same((ids, sc, cnt), want)
        assert st.fallback_queries > 0
        assert_same(host(g.search_tt_device(SHAPE, RANKS, dev_cores(us), 10, 50)), want_u)
        g.set_heap_capacity(results=16)
        ids, sc, cnt, st = g.search_tt(lib_tts(ts), 10, 50, with_stats=True)
        assert_same((ids, sc, cnt), want)
        assert st.fallback_queries == len(ts)
        assert_same(host(g.search_tt_device(SHAPE, RANKS, dev_cores(us), 10, 50)), want_u)
        g.set_heap_capacity()
        ids, sc, cnt, st = g.search_tt(lib_tts(ts), 10, 50, with_stats=True)
        assert_same((ids, sc, cnt), want)
        assert st.fallback_queries == 0


def test_insert_tt_builds_the_oracles_graph():
    from neumann_amd import GpuHnsw
    rng = np.random.default_rng(0x7753)
    ts = [to.random_tt(rng, SHAPE, RANKS if i % 4 else [1, 1, 2, 1]) for i in range(120)]
    for metric in (ho.COSINE, ho.EUCLIDEAN):
        o = ho.HNSWIndex(o_cfg(metric))
        for t in ts:
            to.insert_tt_vector(o, t)
        with GpuHnsw(DIM, g_cfg(metric)) as g:
            assert g.insert_tt(lib_tts(ts[:50])).tolist() == list(range(50))
            assert g.insert_tt(lib_tts(ts[50:])).tolist() == list(range(50, 120))
            assert len(g) == len(o) and g.entry_point == o.entry_point and g.max_layer == o.max_layer
            assert g.levels().tolist() == o.levels
            for node in range(len(o)):
                for layer in range(o.levels[node] + 1):
                    assert g.neighbors(node, layer).tolist() == o.neighbors[node][layer], (node, layer)
                assert np.array_equal(bits(g.get_vector(node)), bits(o.rows[node]))
            assert g.memory_stats()["dense_count"] == 120
            assert_same(g.search_tt(lib_tts(ts[:8]), 5), to.answers_tt(o, ts[:8], 5))


def test_refusals_write_nothing():
    import ctypes as C
    from neumann_amd import GpuHnsw, _capi, tt
    lib = _capi.load()
    rows, _ = corpus()
    good = uniform_trains()[:2]

    def call_search(g, shape, ranks, off, cores, nq, k=4):
        shape, ranks = np.asarray(shape, dtype=np.uint32), np.asarray(ranks, dtype=np.uint32)
        off, cores = np.asarray(off, dtype=np.uint64), np.asarray(cores, dtype=F)
        ids = np.full((nq, k), 7, dtype=np.uint64)
        sc = np.full((nq, k), 7, dtype=F)
        cnt = np.full(nq, 7, dtype=np.uint32)
        p = lambda a: C.c_void_p(a.ctypes.data)
        st = lib.nmn_hnsw_search_tt(g._h, p(shape), shape.size, p(ranks), p(off), p(cores), nq, k, 0, p(ids), p(sc), p(cnt), None)
        assert (ids == 7).all() and (sc == 7).all() and (cnt == 7).all()
        return st, lib.nmn_last_error().decode()

    shape, ranks, off, cores = to.pack(good)
    with GpuHnsw(DIM, g_cfg(ho.COSINE)) as g:
        g.insert(rows[:50])
        bad_ranks = ranks.copy()
        bad_ranks[1, 0] = 2
        st, text = call_search(g, shape, bad_ranks, off, cores, 2)
        assert st == _capi.ERR_INVALID_ARGUMENT and "query 1" in text and "ranks[0]" in text
        bad_ranks = ranks.copy()
        bad_ranks[1, 1] = 0
        st, text = call_search(g, shape, bad_ranks, off, cores, 2)
        assert st == _capi.ERR_INVALID_ARGUMENT and "query 1" in text and ">= 1" in text
        bad_off = off.copy()
        bad_off[2] -= 1
        st, text = call_search(g, shape, ranks, bad_off, cores, 2)
        assert st == _capi.ERR_INVALID_ARGUMENT and "query 1" in text and "core_off" in text
        st, text = call_search(g, [2, 0, 5], ranks, off, cores, 2)
        assert st == _capi.ERR_INVALID_ARGUMENT and "shape" in text
        st, text = call_search(g, [2] * 9, np.ones((2, 10)), off, cores, 2)
        assert st == _capi.ERR_INVALID_ARGUMENT and "n_cores" in text
        st, text = call_search(g, [2, 2, 4], ranks, [0, 20, 40], np.zeros(40), 2)       # well formed, another dimension
        assert st == _capi.ERR_DIMENSION_MISMATCH and "16" in text
        st, text = call_search(g, shape, ranks, off, cores, 2, k=0)
        assert st == _capi.ERR_INVALID_TOP_K
        with pytest.raises(_capi.NeumannGpuError) as e:
            tt.TTVector([2, 2, 5], [1, 2, 2, 2], good[0].cores)
        assert e.value.status == _capi.ERR_INVALID_ARGUMENT
        # the device entry: one train above the LDS limits is refused (rank 33), nothing enqueued
        import torch
        big = torch.zeros((1, 2 * 33 + 33 * 2 * 33 + 33 * 5), dtype=torch.float32, device="cuda")
        with pytest.raises(_capi.NeumannGpuError) as e:
            g.search_tt_device(SHAPE, [1, 33, 33, 1], big, 4)
        assert e.value.status == _capi.ERR_INVALID_ARGUMENT and "LDS" in str(e.value)
        with pytest.raises(_capi.NeumannGpuError) as e:
            g.search_tt_device([2, 2, 4], RANKS, torch.zeros((1, 20), dtype=torch.float32, device="cuda"), 4)
        assert e.value.status == _capi.ERR_DIMENSION_MISMATCH
        # insert_tt: a malformed batch inserts nothing; max_nodes is nmn_hnsw_insert's, all or nothing
        n0 = len(g)
        ids = np.full(2, 7, dtype=np.uint64)
        p = lambda a: C.c_void_p(a.ctypes.data)
        st = lib.nmn_hnsw_insert_tt(g._h, p(shape), 3, p(bad_ranks), p(off), p(cores), 2, p(ids))
        assert st == _capi.ERR_INVALID_ARGUMENT and len(g) == n0 and (ids == 7).all()
    cfg = g_cfg(ho.COSINE)
    cfg.max_nodes = 3
    with GpuHnsw(DIM, cfg) as g:
        g.insert_tt(lib_tts(good))
        with pytest.raises(_capi.NeumannGpuError) as e:
            g.insert_tt(lib_tts(good))
        assert e.value.status == _capi.ERR_CAPACITY and "HNSW index at capacity: 2 nodes (limit: 3)" in str(e.value) and len(g) == 2
    with GpuHnsw(DIM, g_cfg(ho.COSINE), storage="quantized") as g:
        with pytest.raises(_capi.NeumannGpuError) as e:
            g.insert_tt(lib_tts(good))
        assert e.value.status == _capi.ERR_CONFIGURATION and len(g) == 0


def test_eight_threads_half_search_half_search_tt():
    o = oracle("dense", ho.EUCLIDEAN)
    ts = trains()
    rng = np.random.default_rng(31)
    Q = rng.standard_normal((8, DIM)).astype(F)
    want_tt = [to.answers_tt(o, ts[i:i + 3], 10, 50) for i in range(4)]
    want_d = [ho.padded_answers(o, Q[2 * i:2 * i + 2], 10, 50) for i in range(4)]
    got, errors = {}, []
    with gpu_index("dense", ho.EUCLIDEAN) as g:
        def work(i):
            try:
                for _ in range(5):
                    got[i] = g.search_tt(lib_tts(ts[i:i + 3]), 10, 50) if i < 4 else g.search(Q[2 * (i - 4):2 * (i - 4) + 2], 10, 50)
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
