"""nmn_hnsw_search_sparse_device / GpuHnsw.search_sparse_device (docs/hnsw.md §22): the CSR canonicalised on the GPU, then the
sparse walk, all in stream order.  Ids, score BITS and counts against BOTH tests/_hnsw_sparse_query_oracle.py (the mixed oracle
on a handle with sparse nodes) and the product's host-buffer search_sparse.  Corpora, oracles and handles' recipes are those of
tests/test_gpu_hnsw_sparse_query.py and tests/test_gpu_hnsw_mixed.py, shared through their caches."""
import ctypes as C
import threading

import numpy as np
import pytest

from tests import _hnsw_mixed_oracle as mo
from tests import _hnsw_oracle as ho
from tests import _hnsw_sparse_query_oracle as so
from tests import _xmetric_oracle as xo
from tests import test_gpu_hnsw_mixed as mixed
from tests import test_gpu_hnsw_sparse_query as base

pytestmark = pytest.mark.gpu
F = np.float32
NONE64 = np.uint64(0xFFFFFFFFFFFFFFFF)
assert_same = base.assert_same


def dev_csr(csr):
    import torch
    ip, pos, val = csr
    return (torch.from_numpy(np.asarray(ip).astype(np.int64)).cuda(),
            torch.from_numpy(np.ascontiguousarray(pos, dtype=np.uint32).view(np.int32)).cuda(),
            torch.from_numpy(np.ascontiguousarray(val, dtype=F)).cuda())


def host4(res):
    import torch
    torch.cuda.synchronize()
    ids, sc, cnt, status = res
    return ids.cpu().numpy().view(np.uint64), sc.cpu().numpy(), cnt.cpu().numpy().astype(np.uint32), status.cpu().numpy()


def check(g, want, csr, k, ef, max_nnz=None):
    """the device entry against the oracle's answers AND the host entry's; every query served"""
    twin = g.search_sparse(*csr, k, ef, with_stats=True)
    got = host4(g.search_sparse_device(*dev_csr(csr), k, ef, max_nnz=max_nnz))
    assert not got[3].any(), got[3]
    assert_same(got, want)
    assert_same(got, twin)
    return got, twin[3]


def assert_sentinel_rows(got, rows):
    ids, sc, cnt, _ = got
    assert not cnt[rows].any() and (ids[rows] == NONE64).all() and np.isneginf(sc[rows]).all()


def test_golden_corpus():
    from neumann_amd import GpuHnsw, HNSWConfig
    rows, queries = xo.sparse_golden_corpus()
    o = xo.index_from_golden(base.GOLDEN)
    with GpuHnsw(rows.shape[1], HNSWConfig()) as g:
        g.insert(rows)
        csr = g.sparse_from_dense(queries)
        for ef in (50, 200):
            want, _ = base.want_sparse(o, rows.shape[1], csr, 10, ef)
            check(g, want, csr, 10, ef)


@pytest.mark.parametrize("dim", [20, 33])
@pytest.mark.parametrize("storage", base.STORAGES)
@pytest.mark.parametrize("metric", base.METRICS)
def test_metrics_and_storages(metric, storage, dim):
    name = f"mix:300:{dim}"
    o = base.oracle(name, storage, metric)
    with base.gpu_index(name, storage, metric) as g:
        csr = g.sparse_from_dense(base.corpus(name)[1])
        check(g, base.want_sparse(o, dim, csr, 10, 50)[0], csr, 10, 50)
        check(g, base.want_sparse(o, dim, csr, 305, None)[0], csr, 305, None)   # k > n: ef = k


@pytest.mark.parametrize("dim", [5, 8, 128, 771])
def test_dimensions_cosine_dense(dim):
    name = f"mix:200:{dim}"
    o = base.oracle(name, "dense", ho.COSINE)
    Q = base.corpus(name)[1].copy()
    Q[4] = base.corpus(name)[0][3]
    Q[4][Q[4] == 0] = F(0.5)                                  # every position stored
    with base.gpu_index(name, "dense", ho.COSINE) as g:
        csr = g.sparse_from_dense(Q)
        check(g, base.want_sparse(o, dim, csr, 10, 50)[0], csr, 10, 50)


@pytest.mark.parametrize("storage", base.STORAGES)
@pytest.mark.parametrize("metric", base.METRICS)
def test_special_queries_in_one_call(metric, storage):
    """entry-less, one entry, every position, unsorted with zeros of both signs and one position three times, zeros only — on the
    corpus with duplicate and zero rows.  No handle here holds sparse nodes, so the duplicated position is served."""
    name = "special:240:12"
    o = base.oracle(name, storage, metric)
    csr = base.special_csr(12, base.corpus(name)[0])
    with base.gpu_index(name, storage, metric) as g:
        check(g, base.want_sparse(o, 12, csr, 10, 50)[0], csr, 10, 50)
        check(g, base.want_sparse(o, 12, csr, 10, 50)[0], csr, 10, 50, max_nnz=4096)   # the largest query region: the same answers


@pytest.mark.parametrize("storage,metric", [("dense", ho.COSINE), ("dense", ho.DOT_PRODUCT), ("quantized", ho.COSINE)])
def test_overflow_paths(storage, metric):
    """both overflow paths apply unchanged; fallback_queries is seen through the host twin of the same call"""
    name = "mix:300:20"
    o = base.oracle(name, storage, metric)
    with base.gpu_index(name, storage, metric) as g:
        csr = g.sparse_from_dense(base.corpus(name)[1])
        want = base.want_sparse(o, 20, csr, 10, 50)[0]
        g.set_heap_capacity(results=0, candidates=16)
        assert check(g, want, csr, 10, 50)[1].fallback_queries > 0
        g.set_heap_capacity(results=16)
        assert check(g, want, csr, 10, 50)[1].fallback_queries == len(csr[0]) - 1
        g.set_heap_capacity()
        assert check(g, want, csr, 10, 50)[1].fallback_queries == 0


def test_empty_and_single_node():
    from neumann_amd import GpuHnsw
    csr = (np.array([0, 1, 1], np.uint64), np.array([2], np.uint32), np.array([1.0], F))
    with GpuHnsw(6, base.g_cfg(ho.COSINE)) as g:
        got = host4(g.search_sparse_device(*dev_csr(csr), 3))                               # n = 0
        assert not got[3].any()
        assert_sentinel_rows(got, [0, 1])
        assert_same(got, g.search_sparse(*csr, 3))
        row = np.arange(6, dtype=F)[None, :]
        g.insert(row)                                                                        # n = 1
        o = ho.build(row, base.o_cfg(ho.COSINE))
        check(g, base.want_sparse(o, 6, csr, 3, None)[0], csr, 3, None)


@pytest.mark.parametrize("metric", [ho.COSINE, ho.DOT_PRODUCT])
def test_mixed_handle_and_status_3(metric):
    """a handle with sparse nodes: the MIX walk; there a query with a duplicated position is status 3 — its row the sentinels, its
    neighbours intact — while an all-dense handle serves the same query"""
    name = "inter:200:20"
    o = mixed.oracle(name, metric)
    Q = mixed.corpus(name)[2]
    sqs = [mo.SparseVector.from_dense(q) for q in Q]
    dup = so.SparseQuery.from_parts(20, [7, 2, 9, 2, 0, 4, 2], [1.5, -3.0, 0.5, 4.0, -0.0, 0.25, -8.0])
    with mixed.gpu_index(name, metric) as g:
        csr = mo.csr_of(sqs)
        check(g, mo.answers_sparse(o, sqs, 10, 50), csr, 10, 50)
        # the duplicated query between two others, raw (unsorted, a zero): only the device knows it has a duplicate
        parts = [(sqs[0].positions, sqs[0].values), ([7, 2, 9, 2, 0, 4, 2], [1.5, -3.0, 0.5, 4.0, -0.0, 0.25, -8.0]),
                 (sqs[9].positions, sqs[9].values)]
        indptr = np.cumsum([0] + [len(p) for p, _ in parts]).astype(np.uint64)
        raw = (indptr, np.array([x for p, _ in parts for x in p], np.uint32), np.concatenate([np.asarray(v, F) for _, v in parts]))
        got = host4(g.search_sparse_device(*dev_csr(raw), 10, 50))
        assert got[3].tolist() == [0, 3, 0]
        assert_sentinel_rows(got, [1])
        want = mo.answers_sparse(o, [sqs[0], sqs[9]], 10, 50)
        assert_same(tuple(a[[0, 2]] for a in got[:3]), want)
    # the same three queries on an all-dense handle over the same rows: every one served, the duplicate included
    rows = mixed.corpus(name)[0]
    od = ho.build(rows, mixed.o_cfg(metric))
    from neumann_amd import GpuHnsw
    with GpuHnsw(20, mixed.g_cfg(metric)) as gd:
        gd.insert(rows)
        want = so.padded_answers(od, [sqs[0], dup, sqs[9]], 10, 50)[0]
        check(gd, want, raw, 10, 50)


def test_statuses_1_and_2_inside_a_call():
    name = "mix:300:20"
    o = base.oracle(name, "dense", ho.COSINE)
    Q = base.corpus(name)[1]
    with base.gpu_index(name, "dense", ho.COSINE) as g:
        ip, pos, val = g.sparse_from_dense(Q[:6])
        ip = ip.astype(np.int64)
        want = base.want_sparse(o, 20, (ip, pos, val), 10, 50)[0]
        bad_pos = pos.copy()
        bad_pos[ip[1]] = 20                                     # query 1: a position == dim
        bad_ip = ip.copy()
        bad_ip[4] = ip[3] - 1                                   # query 3 ends before it starts: status 2 (query 4 begins one entry
        served = [0, 2, 5]                                      # early and is another query: not compared)
        got = host4(g.search_sparse_device(*dev_csr((bad_ip, bad_pos, val)), 10, 50))
        assert got[3][[0, 1, 2, 3, 5]].tolist() == [0, 1, 0, 2, 0]
        assert_sentinel_rows(got, [1, 3])
        assert_same(tuple(a[served] for a in got[:3]), tuple(a[served] for a in want))
        far_ip = ip.copy()
        far_ip[6] = len(pos) + 1                                # the last range runs past nnz_total
        import torch
        ids = torch.full((6, 10), 77, dtype=torch.int64, device="cuda")
        sc = torch.full((6, 10), 7.0, dtype=torch.float32, device="cuda")
        cnt = torch.full((6,), 99, dtype=torch.int32, device="cuda")
        # status not asked for (a null pointer): the same rows, simply not reported
        d = dev_csr((far_ip, pos, val))
        st = g._lib.nmn_hnsw_search_sparse_device(g._h, *[C.c_void_p(t.data_ptr()) for t in d], 6, len(pos), 0,
                                                  10, 50, C.c_void_p(ids.data_ptr()), C.c_void_p(sc.data_ptr()), C.c_void_p(cnt.data_ptr()),
                                                  None, C.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert st == 0
        got = host4((ids, sc, cnt, cnt))
        assert_sentinel_rows(got, [5])
        assert_same(tuple(a[:5] for a in got[:3]), tuple(a[:5] for a in want))


def test_configuration_refusals_write_nothing():
    """a binary handle; sparse nodes under Euclidean; a sparse node with a duplicated position: NMN_ERR_CONFIGURATION, the text names
    the reason, the pre-filled outputs are found as they were"""
    import torch
    from neumann_amd import GpuHnsw, NeumannGpuError, _capi
    rng = np.random.default_rng(3)
    rows = rng.standard_normal((12, 8)).astype(F)
    csr = (np.array([0, 2], np.uint64), np.array([1, 5], np.uint32), np.array([1.0, -2.0], F))

    def refused(g, word):
        out = (torch.full((1, 3), 77, dtype=torch.int64, device="cuda"), torch.full((1, 3), 7.0, dtype=torch.float32, device="cuda"),
               torch.full((1,), 99, dtype=torch.int32, device="cuda"))
        status = torch.full((1,), 55, dtype=torch.int32, device="cuda")
        with pytest.raises(NeumannGpuError) as e:
            g.search_sparse_device(*dev_csr(csr), 3, out=out, status=status)
        assert e.value.status == _capi.ERR_CONFIGURATION and word in str(e.value), str(e.value)
        torch.cuda.synchronize()
        assert (out[0] == 77).all() and (out[1] == 7.0).all() and (out[2] == 99).all() and (status == 55).all()

    with GpuHnsw(8, base.g_cfg(ho.COSINE), storage="binary") as g:
        g.insert(rows)
        refused(g, "Binary")
    with GpuHnsw(8, base.g_cfg(ho.EUCLIDEAN)) as g:
        g.insert(rows)
        g.insert_sparse([0, 2], [1, 4], [1.0, 2.0])
        refused(g, "Euclidean")
    with GpuHnsw(8, base.g_cfg(ho.COSINE)) as g:
        g.insert(rows)
        g.insert_sparse([0, 3], [1, 4, 1], [1.0, 2.0, 3.0])
        refused(g, "duplicated position")


def test_search_then_insert_without_a_synchronise():
    """nmn_hnsw_insert waits for the device search in flight: the answers are those of the index before the insert"""
    import torch
    name = "mix:300:20"
    rows, Q = base.corpus(name)
    big = np.tile(Q, (40, 1))                                  # 960 queries: the walk is still running when insert is called
    with base.gpu_index(name, "dense", ho.COSINE) as g:
        csr = g.sparse_from_dense(big)
        before = g.search_sparse(*csr, 10, 50)
        d = dev_csr(csr)
        torch.cuda.synchronize()
        res = g.search_sparse_device(*d, 10, 50)
        g.insert(Q[:8])                                        # no synchronise in between; the queries themselves become nodes
        got = host4(res)
        assert not got[3].any()
        assert_same(got, before)
        after = g.search_sparse(*csr, 10, 50)
        assert not np.array_equal(after[0], before[0])         # ... and the insert did change the answers


def test_four_streams_beside_a_host_caller():
    import torch
    name = "mix:300:20"
    Q = base.corpus(name)[1]
    with base.gpu_index(name, "dense", ho.COSINE) as g:
        parts = [g.sparse_from_dense(Q[6 * t: 6 * t + 6]) for t in range(4)]
        alone = [g.search_sparse(*p, 10, 50) for p in parts]
        whole = g.sparse_from_dense(Q)
        alone_host = g.search_sparse(*whole, 10, 50)
        devs = [dev_csr(p) for p in parts]
        # every thread's outputs are made here and reused by its calls: a tensor torch frees while a call on another stream still
        # writes it would be handed to the next allocation of any thread
        outs = [(torch.empty((6, 10), dtype=torch.int64, device="cuda"), torch.empty((6, 10), dtype=torch.float32, device="cuda"),
                 torch.empty((6,), dtype=torch.int32, device="cuda"), torch.empty((6,), dtype=torch.int32, device="cuda")) for _ in range(4)]
        torch.cuda.synchronize()
        out, errs = [None] * 5, []

        def run(t):
            try:
                if t == 4:
                    for _ in range(5):
                        out[4] = g.search_sparse(*whole, 10, 50)
                    return
                s = torch.cuda.Stream()
                for _ in range(5):
                    res = g.search_sparse_device(*devs[t], 10, 50, out=outs[t][:3], status=outs[t][3], stream=s)
                s.synchronize()
                out[t] = tuple(x.cpu() for x in res)
            except Exception as e:  # noqa: BLE001
                errs.append(e)

        threads = [threading.Thread(target=run, args=(t,)) for t in range(5)]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
        assert not errs, errs
        for t in range(4):
            got = host4(out[t])
            assert not got[3].any()
            assert_same(got, alone[t])
        assert_same(out[4], alone_host)
