"""IVF-Binary on the GPU (nmn_ivf_build_ex / nmn_ivf_create_ex with NMN_IVF_BINARY) against tests/_ivf_codec_oracle.py, the
numpy restatement of tensor_store/src/binary_quantization.rs and the Binary branches of ivf.rs: identical bit-words, identical
ids in identical order with bit-equal distances.  Distances take only dim + 1 values, so ties are the normal case."""
import threading

import numpy as np
import pytest

from tests import _ivf_codec_oracle as co

pytestmark = pytest.mark.gpu
F = np.float32
NONE = np.uint64(0xFFFFFFFFFFFFFFFF)
FAST = dict(max_iterations=2, convergence_threshold=1.0, seed=42, init_method="random")  # ivf.rs:589-596
METHODS = ["sign", "mean", "median"]


def data(n, d, seed=0, blobs=8):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((n, d)) + 3.0 * rng.standard_normal((blobs, d))[rng.integers(0, blobs, n)]).astype(F)


def pair(V, C, method, nprobe=None, spare=64):
    from neumann_amd.ivf import GpuIvfBinary
    orc = co.IVFCoded(C, "binary", threshold=method, nprobe=nprobe, kmeans=co.KMeansConfig(**FAST))
    orc.train(V)
    gpu = GpuIvfBinary(orc.centroids, capacity_rows=len(V) + spare, threshold=method, nprobe=orc.nprobe)
    return orc, gpu


def check_search(orc, gpu, Q, k, nprobe=None):
    Q = np.atleast_2d(Q)
    ids, dist, counts = gpu.search(Q, k, nprobe)
    for i, q in enumerate(Q):
        eids, ed = orc.search(q, k, nprobe)
        assert counts[i] == len(eids)
        assert ids[i, :len(eids)].tolist() == eids
        assert np.array_equal(dist[i, :len(eids)].view(np.uint32), np.asarray(ed, F).view(np.uint32))
        assert np.all(ids[i, len(eids):] == NONE) and np.all(np.isposinf(dist[i, len(eids):]))


def add_both(orc, gpu, V):
    clusters = gpu.add(V)
    for v in V:
        orc.add(v)
    assert clusters.tolist() == orc.assign[-len(V):]


@pytest.mark.parametrize("method", METHODS)
def test_build_words_and_search(method):
    from neumann_amd.ivf import GpuIvfBinary
    V = data(500, 16, seed=1)
    orc = co.IVFCoded(6, "binary", threshold=method, kmeans=co.KMeansConfig(**FAST))
    orc.train(V)
    for v in V:
        orc.add(v)
    with GpuIvfBinary.build(V, 6, threshold=method, **FAST) as gpu:
        assert gpu.storage_kind == 2 and len(gpu) == 500 and gpu.list_major_rows == 500
        assert gpu._lib.nmn_ivf_vectors(gpu._h) is None
        assert np.array_equal(gpu.centroids().view(np.uint32), orc.centroids.view(np.uint32))
        assert np.array_equal(gpu.codes(), np.stack(orc.codes))
        assert gpu.cluster_sizes().tolist() == orc.cluster_sizes()
        Q = data(64, 16, seed=2)
        for nprobe in (1, None, 6):
            for k in (1, 10, 1000):
                for nq in (1, 7, 64):
                    check_search(orc, gpu, Q[:nq], k, nprobe)


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("d", [768, 77])
def test_wide_and_odd_dimensions(method, d):
    V = data(240, d, seed=3)
    V[10:30] = V[9]                                    # duplicates: equal words
    if method == "median":
        V[40, : d // 2] = V[40, d // 2: 2 * (d // 2)]  # repeated values around the middle
    orc, gpu = pair(V, 5, method)
    with gpu:
        add_both(orc, gpu, V)
        assert np.array_equal(gpu.codes(), np.stack(orc.codes))
        Q = np.concatenate([V[9:10], data(6, d, seed=4)])
        check_search(orc, gpu, Q, 60, 3)
        check_search(orc, gpu, Q, 1000, 5)


def test_tie_order_is_probe_rank_then_id():
    V = data(600, 16, seed=5)
    orc, gpu = pair(V, 8, "sign")
    with gpu:
        add_both(orc, gpu, V)
        q = data(1, 16, seed=6)[0]
        ids, dist, counts = gpu.search(q, 600, 8)
        ids, dist = ids[0, :counts[0]], dist[0, :counts[0]]
        cd = co.sq_dist_rows(orc.centroids, q)
        rank = {c: r for r, c in enumerate(sorted(range(8), key=lambda c: float(cd[c])))}
        key = [(float(dd), rank[orc.assign[int(i)]], int(i)) for i, dd in zip(ids, dist)]
        assert key == sorted(key) and len(set(dist.tolist())) <= 17
        check_search(orc, gpu, q, 600, 8)


def test_build_half_then_add_the_rest():
    from neumann_amd.ivf import GpuIvfBinary
    V = data(800, 64, seed=7)
    orc = co.IVFCoded(6, "binary", threshold="mean", kmeans=co.KMeansConfig(**FAST))
    orc.train(V[:400])
    for v in V:
        orc.add(v)
    with GpuIvfBinary.build(V[:400], 6, threshold="mean", capacity_rows=800, **FAST) as gpu:
        gpu.add(V[400:])
        assert np.array_equal(gpu.codes(), np.stack(orc.codes)) and gpu.cluster_sizes().tolist() == orc.cluster_sizes()
        check_search(orc, gpu, data(20, 64, seed=8), 30, 2)


def test_engine_build_and_search_with_ivf(tmp_path):
    from neumann_amd.engine import IVFBuildOptions, VectorEngine, VectorError
    V = data(200, 64, seed=9)
    e = VectorEngine()
    for i, v in enumerate(V):
        e.store_embedding(f"k{i}", v.tolist())
    opt = IVFBuildOptions.binary(4)
    opt.max_iterations, opt.convergence_threshold, opt.init_method = 2, 1.0, "random"
    index, keys = e.build_ivf_index(opt)
    rows = np.array([e.get_embedding(k) for k in keys], dtype=F)
    orc = co.IVFCoded(4, "binary", threshold="sign", kmeans=co.KMeansConfig(**FAST))
    orc.train(rows)
    for v in rows:
        orc.add(v)
    q = V[5]
    res = e.search_with_ivf(index, keys, q.tolist(), 25)
    eids, ed = orc.search(q, 25)
    assert [r.key for r in res] == [keys[i] for i in eids]
    assert [F(r.score) for r in res] == [F(F(1.0) / F(F(1.0) + d)) for d in ed]
    assert e.estimate_ivf_memory(opt) == co.estimate_ivf_memory(200, 64, 4, "binary")
    with pytest.raises(VectorError) as ei:
        e.save_ivf_index(index, tmp_path / "b.idx")
    assert ei.value.kind == "ConfigurationError"


def test_hbm_per_vector_is_the_words():
    from neumann_amd import _capi
    from neumann_amd.ivf import GpuIvfBinary
    C = data(4, 768, seed=10)
    with GpuIvfBinary(C, 1) as a, GpuIvfBinary(C, 100_001) as b:
        assert b.hbm_bytes - a.hbm_bytes == 100_000 * 96
        with pytest.raises(_capi.NeumannGpuError) as ei:
            b.save("/dev/null")
        assert ei.value.status == _capi.ERR_CONFIGURATION


def test_concurrent_searches_equal_sequential():
    V = data(4000, 64, seed=11)
    orc, gpu = pair(V, 16, "median")
    with gpu:
        gpu.add(V)
        Q = data(48, 64, seed=12)
        want = [gpu.search(Q[i], 20, 2 + i % 5) for i in range(48)]
        got = [None] * 48
        errs = []

        def work(t):
            try:
                for j in range(t, 48, 8):
                    got[j] = gpu.search(Q[j], 20, 2 + j % 5)
            except Exception as ex:  # noqa: BLE001
                errs.append(ex)
        th = [threading.Thread(target=work, args=(t,)) for t in range(8)]
        for t in th:
            t.start()
        for t in th:
            t.join()
        assert not errs
        for w, g in zip(want, got):
            assert all(np.array_equal(x, y) for x, y in zip(w, g))
