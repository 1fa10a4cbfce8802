"""IVF-PQ on the GPU (nmn_ivf_build_ex / nmn_ivf_create_ex with NMN_IVF_PQ) against tests/_ivf_codec_oracle.py, the numpy
restatement of tensor_store/src/pq.rs and the PQ branches of ivf.rs: bit-equal codebooks, identical codes, identical ids in
identical order with bit-equal distances."""
import threading

import numpy as np
import pytest

from tests import _ivf_codec_oracle as co

pytestmark = pytest.mark.gpu
F = np.float32
NONE = np.uint64(0xFFFFFFFFFFFFFFFF)
FAST = dict(max_iterations=2, convergence_threshold=1.0, seed=42, init_method="random")  # ivf.rs:589-596
PQ_KM = dict(max_iterations=3, convergence_threshold=1e-4, seed=7, init_method="kmeans++")


def km(d):
    return co.KMeansConfig(**d)


def data(n, d, seed=0, blobs=8):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((n, d)) + 3.0 * rng.standard_normal((blobs, d))[rng.integers(0, blobs, n)]).astype(F)


def pair(V, C, M, K, nprobe=None, spare=64, train=None):
    """oracle trained on `train` (default V) and a GPU index created from ITS centroids and codebook"""
    from neumann_amd.ivf import GpuIvfPQ
    orc = co.IVFCoded(C, "pq", pq_config=co.PQConfig(M, K, km(FAST)), nprobe=nprobe, kmeans=km(FAST))
    orc.train(V if train is None else train)
    gpu = GpuIvfPQ(orc.centroids, orc.codebook.centroids, capacity_rows=len(V) + spare, num_subspaces=M, nprobe=orc.nprobe)
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


@pytest.mark.parametrize("init", ["random", "kmeans++"])
def test_build_codebook_bit_equal(init):
    """nmn_ivf_build_ex trains the IVF centroids and each subspace's codebook with the exact GPU k-means: bit-equal to the
    oracle, with a pq_kmeans that differs from the IVF k-means (seed, iterations, initialisation)."""
    from neumann_amd.ivf import GpuIvfPQ
    V = data(400, 16, seed=1)
    ivf_km = dict(max_iterations=4, convergence_threshold=1e-4, seed=3, init_method=init)
    pq_km = dict(PQ_KM, init_method="random" if init == "kmeans++" else "kmeans++")
    orc = co.IVFCoded(6, "pq", pq_config=co.PQConfig(4, 12, km(pq_km)), kmeans=km(ivf_km))
    orc.train(V)
    for v in V:
        orc.add(v)
    with GpuIvfPQ.build(V, 6, num_subspaces=4, num_centroids=12, pq_kmeans=pq_km, **ivf_km) as gpu:
        assert gpu.storage_kind == 1 and len(gpu) == 400 and gpu.num_codewords == 12
        assert np.array_equal(gpu.centroids().view(np.uint32), orc.centroids.view(np.uint32))
        assert np.array_equal(gpu.codebook().view(np.uint32), orc.codebook.centroids.view(np.uint32))
        assert np.array_equal(gpu.codes(), np.stack(orc.codes))
        assert gpu.cluster_sizes().tolist() == orc.cluster_sizes()
        assert gpu.list_major_rows == 400
        assert gpu._lib.nmn_ivf_vectors(gpu._h) is None  # no f32 rows on the device
        check_search(orc, gpu, V[:7] + F(0.25), 10)


def test_codes_and_search_grid():
    V = data(1500, 32, seed=2)
    orc, gpu = pair(V, 12, 8, 32)
    with gpu:
        add_both(orc, gpu, V)
        assert np.array_equal(gpu.codes(), np.stack(orc.codes))
        Q = data(64, 32, seed=3)
        for nprobe in (1, None, 12):
            for k in (1, 10, 1000, 5000):
                for nq in (1, 7, 64):
                    check_search(orc, gpu, Q[:nq], k, nprobe)


def test_ties_small_codebook_and_duplicates():
    """K = 4: few distinct distances, runs of equal distances across lists; duplicated vectors: equal codes in one list.
    Equal distances keep (probe rank, id) order."""
    V = data(800, 16, seed=4)
    V[100:160] = V[99]
    orc, gpu = pair(V, 8, 4, 4)
    with gpu:
        add_both(orc, gpu, V)
        Q = np.concatenate([V[99:100], data(9, 16, seed=5)])
        for nprobe in (1, 3, 8):
            check_search(orc, gpu, Q, 300, nprobe)
        ids, dist, counts = gpu.search(V[99], 800, 8)
        ids, dist = ids[0, :counts[0]], dist[0, :counts[0]]
        cd = co.sq_dist_rows(orc.centroids, V[99])
        rank = {c: r for r, c in enumerate(sorted(range(8), key=lambda c: float(cd[c])))}
        key = [(float(d), rank[orc.assign[int(i)]], int(i)) for i, d in zip(ids, dist)]
        assert key == sorted(key) and len(set(dist.tolist())) < len(dist)


def test_codes_wrap_above_256_codewords():
    V = data(700, 8, seed=6)
    orc, gpu = pair(V, 2, 2, 300)
    with gpu:
        assert gpu.num_codewords == 300
        add_both(orc, gpu, V)
        assert np.array_equal(gpu.codes(), np.stack(orc.codes))
        check_search(orc, gpu, data(7, 8, seed=7), 50, 2)


def test_codewords_clamped_and_zero():
    from neumann_amd.ivf import GpuIvfPQ
    V = data(60, 16, seed=8)
    with GpuIvfPQ.build(V, 4, num_subspaces=4, num_centroids=256, pq_kmeans=FAST, **FAST) as gpu:  # K' = min(256, n)
        assert gpu.num_codewords == 60 and gpu.codebook().shape == (4, 60, 4)
        orc = co.IVFCoded(4, "pq", pq_config=co.PQConfig(4, 256, km(FAST)), kmeans=km(FAST))
        orc.train(V)
        for v in V:
            orc.add(v)
        assert np.array_equal(gpu.codebook().view(np.uint32), orc.codebook.centroids.view(np.uint32))
        check_search(orc, gpu, V[:3], 20, 4)
    with GpuIvfPQ.build(V, 4, num_subspaces=4, num_centroids=0, **FAST) as gpu:  # K' = 0: an empty ADC table
        assert gpu.num_codewords == 0 and not gpu.codes().any()
        ids, dist, counts = gpu.search(V[0], 100, 4)
        assert counts[0] == 60 and np.all(dist[0, :60] == np.sqrt(np.finfo(F).max))
        orc = co.IVFCoded(4, "pq", pq_config=co.PQConfig(4, 0, km(FAST)), kmeans=km(FAST))
        orc.train(V)
        for v in V:
            orc.add(v)
        check_search(orc, gpu, V[:7], 100, 4)  # every distance equal: candidate order (probe rank, id)


def test_dim_not_divisible_is_a_configuration_error():
    from neumann_amd import _capi
    from neumann_amd.ivf import GpuIvfPQ
    with pytest.raises(_capi.NeumannGpuError) as ei:
        GpuIvfPQ.build(data(50, 18, seed=9), 4, num_subspaces=8, **FAST)
    assert ei.value.status == _capi.ERR_CONFIGURATION


@pytest.mark.parametrize("M", [1, 16])
def test_one_subspace_and_one_dimension_per_subspace(M):
    V = data(300, 16, seed=10)
    orc, gpu = pair(V, 4, M, 16)
    with gpu:
        add_both(orc, gpu, V)
        assert np.array_equal(gpu.codes(), np.stack(orc.codes))
        check_search(orc, gpu, data(7, 16, seed=11), 25, 2)


def test_build_half_then_add_the_rest():
    from neumann_amd.ivf import GpuIvfPQ
    V = data(900, 16, seed=12)
    orc = co.IVFCoded(6, "pq", pq_config=co.PQConfig(4, 16, km(FAST)), kmeans=km(FAST))
    orc.train(V[:450])
    for v in V:
        orc.add(v)
    with GpuIvfPQ.build(V[:450], 6, num_subspaces=4, num_centroids=16, pq_kmeans=FAST, capacity_rows=900, **FAST) as gpu:
        gpu.add(V[450:700])
        gpu.add(V[700:])
        assert len(gpu) == 900 and np.array_equal(gpu.codes(), np.stack(orc.codes))
        assert gpu.cluster_sizes().tolist() == orc.cluster_sizes()
        check_search(orc, gpu, data(64, 16, seed=13), 40, 3)


def test_engine_build_and_search_with_ivf():
    from neumann_amd.engine import IVFBuildOptions, KMeansConfig, PQConfig, VectorEngine
    V = data(300, 16, seed=14)
    e = VectorEngine()
    for i, v in enumerate(V):
        e.store_embedding(f"k{i}", v.tolist())
    opt = IVFBuildOptions.pq(5, PQConfig(4, 8, KMeansConfig(**PQ_KM)))
    opt.max_iterations, opt.convergence_threshold, opt.init_method = 3, 1e-4, "random"
    index, keys = e.build_ivf_index(opt)
    orc = co.IVFCoded(5, "pq", pq_config=co.PQConfig(4, 8, km(PQ_KM)),
                      kmeans=co.KMeansConfig(max_iterations=3, convergence_threshold=1e-4, seed=42, init_method="random"))
    rows = np.array([e.get_embedding(k) for k in keys], dtype=F)
    orc.train(rows)
    for v in rows:
        orc.add(v)
    q = V[3] + F(0.1)
    res = e.search_with_ivf(index, keys, q.tolist(), 12)
    eids, ed = orc.search(q, 12)
    assert [r.key for r in res] == [keys[i] for i in eids]
    assert [F(r.score) for r in res] == [F(F(1.0) / F(F(1.0) + d)) for d in ed]
    assert e.estimate_ivf_memory(opt) == co.estimate_ivf_memory(300, 16, 5, "pq", 4)
    from neumann_amd.engine import VectorError
    with pytest.raises(VectorError) as ei:
        e.save_ivf_index(index, "/dev/null/x")
    assert ei.value.status == -6 and ei.value.kind == "ConfigurationError"


def test_hbm_per_vector_is_the_codes_and_save_is_refused(tmp_path):
    """a PQ index keeps M bytes per vector on the device and nothing else that grows with it; no f32 rows"""
    from neumann_amd import _capi
    from neumann_amd.ivf import GpuIvfPQ
    V = data(200, 64, seed=15)
    orc = co.IVFCoded(4, "pq", pq_config=co.PQConfig(8, 16, km(FAST)), kmeans=km(FAST))
    orc.train(V)
    with GpuIvfPQ(orc.centroids, orc.codebook.centroids, 1, num_subspaces=8) as a, \
            GpuIvfPQ(orc.centroids, orc.codebook.centroids, 1_000_001, num_subspaces=8) as b:
        assert b.hbm_bytes - a.hbm_bytes == 1_000_000 * 8
        b.add(V)
        assert b.hbm_bytes - a.hbm_bytes < 1_000_000 * 8 + (8 << 20)  # (+ search scratch once searched)
        with pytest.raises(_capi.NeumannGpuError) as ei:
            b.save(tmp_path / "pq.idx")
        assert ei.value.status == -6 and not (tmp_path / "pq.idx").exists()


def test_concurrent_searches_equal_sequential():
    V = data(3000, 32, seed=16)
    orc, gpu = pair(V, 16, 8, 32)
    with gpu:
        gpu.add(V)
        Q = data(48, 32, seed=17)
        want = [gpu.search(Q[i], 15, 2 + i % 5) for i in range(48)]
        got = [None] * 48
        errs = []

        def work(t):
            try:
                for j in range(t, 48, 8):
                    got[j] = gpu.search(Q[j], 15, 2 + j % 5)
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
