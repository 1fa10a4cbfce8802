"""nmn_ivf_search_device (GpuIvfFlat / GpuIvfPQ / GpuIvfBinary.search_device): the stream-ordered IVF search against the host
call nmn_ivf_search — ids, distance bits and counts identical — and, on small indexes, against the oracles the host call is
proven on (oracle/ivf_oracle.py, tests/_ivf_codec_oracle.py)."""
import threading

import numpy as np
import pytest

from oracle import ivf_oracle as io
from tests import _ivf_codec_oracle as co

pytestmark = pytest.mark.gpu
F = np.float32
NONE = np.uint64(0xFFFFFFFFFFFFFFFF)
FAST = dict(max_iterations=2, convergence_threshold=1.0, seed=42, init_method="random")
SLEEP = 40_000_000  # torch.cuda._sleep cycles: tens of milliseconds, bounded


def data(n, d, seed=0, blobs=8):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((n, d)) + 3.0 * rng.standard_normal((blobs, d))[rng.integers(0, blobs, n)]).astype(F)


def dev(Q):
    import torch
    return torch.from_numpy(np.ascontiguousarray(np.atleast_2d(Q), dtype=F)).cuda()


def host(res):
    ids, dist, counts = res
    return ids.cpu().numpy().view(np.uint64), dist.cpu().numpy(), counts.cpu().numpy().astype(np.uint32)


def assert_same(a, b):
    """(ids, distances, counts) pairs equal: ids, distance BITS, counts"""
    ia, da, ca = a
    ib, db, cb = b
    assert np.array_equal(ca, cb), (ca, cb)
    assert np.array_equal(ia, ib)
    assert np.array_equal(np.ascontiguousarray(da).view(np.uint32), np.ascontiguousarray(db).view(np.uint32))


def check(gpu, Q, k, nprobe=None, stream=None):
    import torch
    Q = np.atleast_2d(np.asarray(Q, F))
    want = gpu.search(Q, k, nprobe)
    got = gpu.search_device(dev(Q), k, nprobe, stream=stream)
    torch.cuda.synchronize()
    assert_same(host(got), want)
    return want


def build(kind, V, C, **kw):
    from neumann_amd.ivf import GpuIvfBinary, GpuIvfFlat, GpuIvfPQ
    if kind == "flat":
        return GpuIvfFlat.build(V, C, **FAST, **kw)
    if kind.startswith("pq"):
        return GpuIvfPQ.build(V, C, num_subspaces=int(kind[2:]), num_centroids=64, pq_kmeans=dict(FAST), **FAST, **kw)
    return GpuIvfBinary.build(V, C, threshold=kind.split("-")[1], **FAST, **kw)


KINDS = ["flat", "pq8", "pq32", "bin-sign", "bin-mean", "bin-median"]


@pytest.mark.parametrize("kind", KINDS)
def test_device_equals_host_call(kind):
    """every nq / k / nprobe of the issue's grid: k below and above the 4096 of the one-workgroup select, beyond the candidates"""
    V = data(6000, 64, seed=1)
    Q = data(100, 64, seed=2)
    with build(kind, V, 16) as gpu:
        C = gpu.n_clusters
        for nq in (1, 3, 64, 100):
            for k in (1, 10, 100, 5000, 6100):
                for nprobe in (1, 8, C, C + 5):
                    if nq == 100 and k >= 5000 and nprobe != C:
                        continue  # (the large-k sort per query: the others cover it)
                    check(gpu, Q[:nq], k, nprobe)


@pytest.mark.parametrize("kind", ["flat", "pq8", "bin-sign"])
def test_empty_index_and_nprobe_zero(kind):
    import torch
    from neumann_amd.ivf import GpuIvfBinary, GpuIvfFlat, GpuIvfPQ
    cents = data(4, 16, seed=3)
    if kind == "flat":
        gpu = GpuIvfFlat(cents, capacity_rows=64, nprobe=2)
    elif kind == "pq8":
        gpu = GpuIvfPQ(cents, data(8 * 4, 2, seed=4).reshape(8, 4, 2), capacity_rows=64, num_subspaces=8, nprobe=2)
    else:
        gpu = GpuIvfBinary(cents, capacity_rows=64, nprobe=2)
    with gpu:
        Q = data(5, 16, seed=5)
        ids, dist, counts = gpu.search_device(dev(Q), 7)
        torch.cuda.synchronize()
        ids, dist, counts = host((ids, dist, counts))
        assert np.all(ids == NONE) and np.all(np.isposinf(dist)) and np.all(counts == 0)
        check(gpu, Q, 7)
        gpu.add(data(40, 16, seed=6))
        ids, dist, counts = host(gpu.search_device(dev(Q), 7, nprobe=0))
        assert np.all(ids == NONE) and np.all(np.isposinf(dist)) and np.all(counts == 0)
        check(gpu, Q, 7, nprobe=0)
        check(gpu, Q, 7)


def test_flat_matches_oracle():
    from neumann_amd.ivf import GpuIvfFlat
    V = data(500, 16, seed=7)
    orc = io.IVFFlat(8, nprobe=3, kmeans=io.KMeansConfig(**FAST))
    orc.train(V)
    for v in V:
        orc.add(v)
    with GpuIvfFlat(orc.centroids, capacity_rows=600, nprobe=3) as gpu:
        gpu.add(V)
        Q = data(6, 16, seed=8)
        ids, dist, counts = host(gpu.search_device(dev(Q), 20))
        for i, q in enumerate(Q):
            eids, ed = orc.search(q, 20)
            assert counts[i] == len(eids) and ids[i, :len(eids)].tolist() == eids
            assert np.array_equal(dist[i, :len(eids)].view(np.uint32), np.asarray(ed, F).view(np.uint32))


@pytest.mark.parametrize("storage", ["pq", "binary"])
def test_codec_matches_oracle(storage):
    from neumann_amd.ivf import GpuIvfBinary, GpuIvfPQ
    V = data(400, 32, seed=9)
    km = co.KMeansConfig(**FAST)
    if storage == "pq":
        orc = co.IVFCoded(8, "pq", pq_config=co.PQConfig(8, 16, km), nprobe=3, kmeans=km)
        orc.train(V)
        gpu = GpuIvfPQ(orc.centroids, orc.codebook.centroids, capacity_rows=500, num_subspaces=8, nprobe=3)
    else:
        orc = co.IVFCoded(8, "binary", threshold="median", nprobe=3, kmeans=km)
        orc.train(V)
        gpu = GpuIvfBinary(orc.centroids, capacity_rows=500, threshold="median", nprobe=3)
    with gpu:
        gpu.add(V)
        for v in V:
            orc.add(v)
        Q = data(5, 32, seed=10)
        ids, dist, counts = host(gpu.search_device(dev(Q), 30))
        for i, q in enumerate(Q):
            eids, ed = orc.search(q, 30)
            assert counts[i] == len(eids) and ids[i, :len(eids)].tolist() == eids
            assert np.array_equal(dist[i, :len(eids)].view(np.uint32), np.asarray(ed, F).view(np.uint32))


def probe_ranks(gpu, q):
    cents = gpu.centroids()
    cd = io.sq_dist_rows(cents, np.asarray(q, F))
    order = sorted(range(len(cd)), key=lambda i: io._sort_key(cd[i]))
    return {c: r for r, c in enumerate(order)}


def assert_candidate_order(ids, dist, count, ranks, assign):
    """equal distances in (probe rank, id) order: the reference's stable sort over the candidates"""
    for j in range(1, count):
        if dist[j] == dist[j - 1]:
            a, b = int(ids[j - 1]), int(ids[j])
            assert (ranks[assign[a]], a) < (ranks[assign[b]], b)
        else:
            assert dist[j] > dist[j - 1]


def test_ties_cut_at_k_flat_small_integers():
    from neumann_amd.ivf import GpuIvfFlat
    rng = np.random.default_rng(11)
    V = rng.integers(-2, 3, (5000, 8)).astype(F)
    cents = V[rng.choice(len(V), 12, replace=False)] + rng.integers(-1, 2, (12, 8)).astype(F) * 0.5
    with GpuIvfFlat(cents, capacity_rows=6000, nprobe=4) as gpu:
        assign = gpu.add(V)
        assert gpu.list_major_rows == 5000
        Q = np.vstack([V[:4], rng.integers(-2, 3, (4, 8)).astype(F)])
        for k in (1, 5, 50, 300, 4096):
            for nprobe in (2, 4, 12):
                want = check(gpu, Q, k, nprobe)
                for i, q in enumerate(Q):
                    assert_candidate_order(want[0][i], want[1][i], want[2][i], probe_ranks(gpu, q), assign)


def test_ties_sign_flipped_copies_zero_query():
    from neumann_amd.ivf import GpuIvfFlat
    rng = np.random.default_rng(12)
    base = rng.standard_normal((300, 8)).astype(F)
    V = np.vstack([base, -base])
    cents = np.vstack([np.eye(8, dtype=F) * s * (1 + 0.1 * i) for i, s in enumerate((1, -1))]).reshape(16, 8)
    with GpuIvfFlat(cents, capacity_rows=700, nprobe=16) as gpu:
        assign = gpu.add(V)
        assert np.mean(assign[:300] != assign[300:]) > 0.9  # a row and its mirror image sit in different lists
        Z = np.zeros((1, 8), F)
        for k in (1, 2, 3, 25, 599, 600, 601):
            for nprobe in (4, 8, 16):
                want = check(gpu, Z, k, nprobe)
                assert_candidate_order(want[0][0], want[1][0], want[2][0], probe_ranks(gpu, Z[0]), assign)


def test_ties_binary_distances():
    from neumann_amd.ivf import GpuIvfBinary
    V = data(5000, 16, seed=13)
    cents = V[:10].copy()
    with GpuIvfBinary(cents, capacity_rows=5000, nprobe=10) as gpu:
        assign = gpu.add(V)
        Q = data(8, 16, seed=14)
        for k in (1, 7, 100, 1000, 4096, 4097):
            want = check(gpu, Q, k)
            for i, q in enumerate(Q):
                assert_candidate_order(want[0][i], want[1][i], want[2][i], probe_ranks(gpu, q), assign)


def test_flat_younger_vectors():
    from neumann_amd.ivf import GpuIvfFlat
    V = data(12000, 24, seed=15)
    Q = data(10, 24, seed=16)
    cents = V[::400][:20].copy()
    with GpuIvfFlat(cents, capacity_rows=12000, nprobe=5) as gpu:
        gpu.add(V[:1000])
        assert gpu.list_major_rows == 0  # no list-major copy yet
        for k in (10, 300):
            check(gpu, Q, k)
        gpu.add(V[1000:6000])
        assert gpu.list_major_rows == 6000
        check(gpu, Q, 10)
        gpu.add(V[6000:6300])  # fewer than an eighth: pending younger vectors
        assert gpu.list_major_rows == 6000 and len(gpu) == 6300
        for k in (10, 300, 5000):
            for nprobe in (1, 5, 20):
                check(gpu, Q, k, nprobe)
        gpu.add(V[6300:])  # a re-layout
        assert gpu.list_major_rows == 12000
        for k in (10, 300):
            check(gpu, Q, k)


@pytest.mark.parametrize("kind", ["flat", "binary"])
def test_more_than_4096_clusters(kind):
    from neumann_amd.ivf import GpuIvfBinary, GpuIvfFlat
    V = data(9000, 8, seed=17)
    cents = data(4500, 8, seed=18)
    gpu = GpuIvfFlat(cents, capacity_rows=9000, nprobe=16) if kind == "flat" else GpuIvfBinary(cents, capacity_rows=9000, nprobe=16)
    with gpu:
        gpu.add(V)
        Q = data(3, 8, seed=19)
        for nprobe in (1, 16, 4500):
            check(gpu, Q, 10, nprobe)
        check(gpu, Q[:1], 5000, 4500)


def test_streams_default_and_two_at_once():
    import torch
    V = data(6000, 32, seed=20)
    Q = data(40, 32, seed=21)
    with build("flat", V, 16) as gpu:
        want = gpu.search(Q, 10)
        check(gpu, Q, 10, stream=torch.cuda.default_stream())
        q1, q2 = dev(Q[:20]), dev(Q[20:])
        torch.cuda.synchronize()
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        with torch.cuda.stream(s1):
            r1 = gpu.search_device(q1, 10)
        with torch.cuda.stream(s2):
            r2 = gpu.search_device(q2, 10)
        torch.cuda.synchronize()
        got = [np.vstack(x) if x[0].ndim == 2 else np.concatenate(x) for x in zip(host(r1), host(r2))]
        assert_same(tuple(got), want)


def test_pipelined_calls_reuse_out():
    import torch
    V = data(6000, 32, seed=22)
    Q = data(50, 32, seed=23)
    with build("pq8", V, 16) as gpu:
        want = [gpu.search(Q[i:i + 1], 10) for i in range(50)]
        qs = [dev(Q[i:i + 1]) for i in range(50)]
        s = torch.cuda.Stream()
        torch.cuda.synchronize()
        kept = []
        with torch.cuda.stream(s):
            out = (torch.empty((1, 10), dtype=torch.int64, device="cuda"), torch.empty((1, 10), dtype=torch.float32, device="cuda"),
                   torch.empty((1,), dtype=torch.int32, device="cuda"))
            for i in range(50):
                r = gpu.search_device(qs[i], 10, out=out)
                assert r[0].data_ptr() == out[0].data_ptr()
                kept.append(tuple(t.clone() for t in r))
        s.synchronize()
        for i in range(50):
            assert_same(host(kept[i]), want[i])


@pytest.mark.parametrize("kind", ["flat", "pq8", "bin-sign"])
def test_call_returns_before_the_device_finishes(kind):
    import torch
    V = data(6000, 32, seed=24)
    Q = data(8, 32, seed=25)
    with build(kind, V, 16) as gpu:
        want = gpu.search(Q, 10)
        q = dev(Q)
        s = torch.cuda.Stream()
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            gpu.search_device(q, 10)  # warm-up: the workspace and the id map exist
            s.synchronize()
            torch.cuda._sleep(SLEEP)
            r = gpu.search_device(q, 10)
            assert not s.query()
        s.synchronize()
        assert_same(host(r), want)


def test_add_waits_for_device_searches_in_flight():
    import torch
    V = data(16000, 32, seed=26)
    Q = data(8, 32, seed=27)
    for kind in ("flat", "pq8"):
        with build(kind, V[:6000], 16, capacity_rows=16000) as gpu:
            before = gpu.search(Q, 20)
            q = dev(Q)
            s = torch.cuda.Stream()
            torch.cuda.synchronize()
            with torch.cuda.stream(s):
                gpu.search_device(q, 20)
                s.synchronize()
                torch.cuda._sleep(SLEEP)
                r = gpu.search_device(q, 20)
            gpu.add(V[6000:])  # enough for a re-layout of the list-major copy / the codes
            if kind == "flat":
                assert gpu.list_major_rows == 16000
            s.synchronize()
            assert_same(host(r), before)
            after = check(gpu, Q, 20)
            assert not np.array_equal(after[0], before[0])


def test_destroy_right_after_enqueue():
    import torch
    V = data(6000, 32, seed=28)
    Q = data(4, 32, seed=29)
    for kind in ("flat", "bin-mean"):
        gpu = build(kind, V, 16)
        want = gpu.search(Q, 10)
        q = dev(Q)
        torch.cuda.synchronize()
        r = gpu.search_device(q, 10)
        gpu.close()
        torch.cuda.synchronize()
        assert_same(host(r), want)


@pytest.mark.parametrize("kind", ["flat", "pq8"])
def test_threads_mix_host_and_device_searches(kind):
    import torch
    V = data(6000, 32, seed=30)
    Q = data(32, 32, seed=31)
    with build(kind, V, 16) as gpu:
        want = [gpu.search(Q[i:i + 4], 10) for i in range(0, 32, 4)]
        errors = []

        def work(t):
            try:
                for it in range(6):
                    j = (t + it) % 8
                    if (t + it) % 2:
                        got = gpu.search(Q[4 * j:4 * j + 4], 10)
                    else:
                        s = torch.cuda.Stream()
                        with torch.cuda.stream(s):
                            r = gpu.search_device(dev(Q[4 * j:4 * j + 4]), 10)
                        s.synchronize()
                        got = host(r)
                    assert_same(got, want[j])
            except Exception as e:  # noqa: BLE001
                errors.append(e)

        th = [threading.Thread(target=work, args=(t,)) for t in range(8)]
        for t in th:
            t.start()
        for t in th:
            t.join()
        assert not errors, errors[0]


def test_errors():
    import torch
    from neumann_amd import _capi
    V = data(500, 16, seed=32)
    with build("flat", V, 4) as gpu:
        with pytest.raises(_capi.NeumannGpuError):
            gpu.search_device(dev(data(2, 8, seed=33)), 5)
        with pytest.raises(_capi.NeumannGpuError):
            gpu.search_device(torch.zeros((2, 16), dtype=torch.float32), 5)
        with pytest.raises(_capi.NeumannGpuError) as ei:
            gpu.search_device(dev(data(2, 16, seed=34)), 0)
        assert ei.value.status == _capi.ERR_INVALID_TOP_K


@pytest.mark.parametrize("kind", ["flat", "pq8", "bin-sign"])
def test_hbm_bytes_grow_only_once_device_searched(kind):
    import torch
    V = data(6000, 32, seed=35)
    with build(kind, V, 16) as a, build(kind, V, 16) as b:
        assert a.hbm_bytes == b.hbm_bytes
        a.search_device(dev(data(2, 32, seed=36)), 10)
        torch.cuda.synchronize()
        assert a.hbm_bytes >= b.hbm_bytes + 6000 * 4


@pytest.mark.parametrize("storage,d", [("flat", 1), ("flat", 17), ("binary", 1), ("binary", 17), ("pq", 4), ("pq", 20)])
def test_padded_stride_matches_oracle(storage, d):
    """A row stride different from the dimension: the queries go through the padding kernel before the centroid sweep, on the
    host call and on the device call of every storage.  Both against the oracles.  (d: the smallest dimension the storage takes
    here — PQ: two subspaces of two — and one whose padded row spans several 8-element groups.)"""
    import torch
    from neumann_amd import GpuFlatIndex
    from neumann_amd.ivf import GpuIvfBinary, GpuIvfFlat, GpuIvfPQ
    with GpuFlatIndex(d, 8) as probe:          # the stride every index of this dimension gets (centroids and vectors alike)
        assert probe.row_stride != d
    V = data(400, d, seed=37)
    km = co.KMeansConfig(**FAST)
    if storage == "flat":
        orc = io.IVFFlat(8, nprobe=3, kmeans=io.KMeansConfig(**FAST))
        orc.train(V)
        gpu = GpuIvfFlat(orc.centroids, capacity_rows=500, nprobe=3)
    elif storage == "pq":
        M = 2 if d == 4 else 4
        orc = co.IVFCoded(8, "pq", pq_config=co.PQConfig(M, 16, km), nprobe=3, kmeans=km)
        orc.train(V)
        gpu = GpuIvfPQ(orc.centroids, orc.codebook.centroids, capacity_rows=500, num_subspaces=M, nprobe=3)
    else:
        orc = co.IVFCoded(8, "binary", threshold="mean", nprobe=3, kmeans=km)
        orc.train(V)
        gpu = GpuIvfBinary(orc.centroids, capacity_rows=500, threshold="mean", nprobe=3)
    with gpu:
        if storage == "flat":
            assert GpuFlatIndex._view(gpu._lib.nmn_ivf_vectors(gpu._h), gpu).row_stride != d
        gpu.add(V)
        for v in V:
            orc.add(v)
        Q = data(5, d, seed=38)
        got_dev = gpu.search_device(dev(Q), 30)
        torch.cuda.synchronize()
        for name, (ids, dist, counts) in (("search", gpu.search(Q, 30)), ("search_device", host(got_dev))):
            for i, q in enumerate(Q):
                eids, ed = orc.search(q, 30)
                assert counts[i] == len(eids) and ids[i, :len(eids)].tolist() == eids, (name, i)
                assert np.array_equal(dist[i, :len(eids)].view(np.uint32), np.asarray(ed, F).view(np.uint32)), (name, i)
