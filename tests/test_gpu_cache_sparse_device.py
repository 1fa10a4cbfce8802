"""nmn_hnsw_cache_search_sparse_device / GpuHnsw.cache_search_sparse_device (docs/hnsw.md §22): canonicalise, sparse walk, re-rank
and filtered ordering as one stream-ordered chain.  Against the product's cache_search_sparse — the same kernels behind the same
candidates, so the BITS of every similarity, Angular / Geodesic included — and against tests/_cache_index_oracle.py under the rule
of tests/test_gpu_hnsw_cache_search.py (bits; 2^-22 for the two acos metrics).  The handles, their dead nodes and their queries are
that file's, shared through its cache; the nine metrics are those of tests/test_gpu_cache_index.py."""
import math

import numpy as np
import pytest

from tests import _cache_index_oracle as co
from tests import _hnsw_mixed_oracle as mo
from tests import _hnsw_oracle as ho
from tests import test_gpu_hnsw_cache_search as base

pytestmark = pytest.mark.gpu
F = np.float32
NONE64 = np.uint64(0xFFFFFFFFFFFFFFFF)
NINE = base.NINE


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
    return ids.cpu().numpy().view(np.uint64), sc.cpu().numpy(), cnt.cpu().numpy().view(np.uint32), status.cpu().numpy()


def same_bits(got, twin, what):
    assert got[2].tolist() == twin[2].tolist(), (what, got[2], twin[2])
    assert np.array_equal(got[0], twin[0]), what
    assert np.array_equal(base.bits(got[1]), base.bits(twin[1])), what


def check(o, g, is_live, sqs, k, thr, metric, what):
    """the three queries in ONE call: device chain == host entry (bits) == oracle (assert_answers' rule); every query served"""
    gm, csr = base.g_metric(metric), mo.csr_of(sqs)
    got = host4(g.cache_search_sparse_device(*dev_csr(csr), k, thr, gm))
    assert not got[3].any(), (what, got[3])
    same_bits(got, g.cache_search_sparse(*csr, k, thr, gm), what)
    base.assert_answers(metric, got, [co.search_nodes_sparse(o, is_live, s, k, thr, metric) for s in sqs], k, what)
    return got


@pytest.mark.parametrize("dim", [20, 33])
@pytest.mark.parametrize("hnsw_metric", [ho.COSINE, ho.EUCLIDEAN, ho.DOT_PRODUCT])
def test_all_dense_handle_nine_metrics(hnsw_metric, dim):
    """dead nodes in the live mask, a threshold that cuts, and — the third query — a duplicated position, scored on its entries by the
    merge kernel while the two others are scored as their to_dense() rows"""
    o, g, live, _, sqs = base.shaped(hnsw_metric, dim, "dense")
    assert len(sqs) == 3 and len(set(sqs[2].positions)) < len(sqs[2].positions)
    is_live = lambda n: bool(live[n])  # noqa: E731
    cut = 0
    for mi, metric in enumerate(NINE):
        k = (1, 4, 7)[mi % 3]
        thr = -math.inf if metric.kind in base.ACOS else 0.2
        got = check(o, g, is_live, sqs, k, thr, metric, f"hnsw={hnsw_metric} d={dim} {metric} k={k}")
        if thr > -math.inf:
            loose = host4(g.cache_search_sparse_device(*dev_csr(mo.csr_of(sqs)), k, -math.inf, base.g_metric(metric)))
            cut += int((got[2] < loose[2]).any())
    assert cut > 0                                   # the threshold did cut somewhere
    assert not live.all()                            # ... and the mask holds dead nodes


@pytest.mark.parametrize("hnsw_metric", [ho.COSINE, ho.DOT_PRODUCT])
def test_mixed_handle(hnsw_metric):
    """sparse nodes (none with a duplicated position) beside dense ones, some dead: served queries against the host entry and the oracle;
    the query with a duplicated position is status 3 there — a sentinel row, the rows beside it intact"""
    rng = np.random.default_rng(100 + hnsw_metric)
    dim, n = 20, 160
    rows = rng.standard_normal((n, dim)).astype(F)
    rows[rng.random(rows.shape) < 0.55] = 0.0
    items = [mo.SparseVector.from_dense(r) if i % 2 else r for i, r in enumerate(rows)]
    o, g = base.build_pair(items, ho.HNSWConfig(**base.SMALL).with_distance_metric(hnsw_metric), dim)
    with g:
        dead = np.flatnonzero(rng.random(n) < 0.15)
        g.set_node_mask(dead, False)
        dead_set = set(dead.tolist())
        is_live = lambda node: node not in dead_set  # noqa: E731
        Q = rng.standard_normal((3, dim)).astype(F)
        Q[rng.random(Q.shape) < 0.6] = 0.0
        sqs = [mo.SparseVector.from_dense(q) for q in Q]
        for metric in (NINE[0], NINE[1], NINE[5], NINE[8]):
            thr = -math.inf if metric.kind in base.ACOS else 0.1
            check(o, g, is_live, sqs, 4, thr, metric, f"mixed hnsw={hnsw_metric} {metric}")
        dup = base.with_duplicate(rng, sqs[0])
        three = [sqs[1], dup, sqs[2]]
        got = host4(g.cache_search_sparse_device(*dev_csr(mo.csr_of(three)), 4, 0.1, base.g_metric(NINE[0])))
        assert got[3].tolist() == [0, 3, 0]
        assert got[2][1] == 0 and (got[0][1] == NONE64).all() and np.isneginf(got[1][1]).all()
        base.assert_answers(NINE[0], tuple(a[[0, 2]] for a in got[:3]),
                            [co.search_nodes_sparse(o, is_live, s, 4, 0.1, NINE[0]) for s in (sqs[1], sqs[2])], 4, "beside status 3")


def test_statuses_and_refusals():
    """statuses 1 and 2 give sentinel rows beside a served query; what nmn_hnsw_cache_search refuses (a quantized handle) and what
    nmn_hnsw_search_sparse_device refuses (sparse nodes under Euclidean) is refused here, with nothing written"""
    import torch
    from neumann_amd import ExtendedDistanceMetric, GpuHnsw, NeumannGpuError, _capi
    o, g, live, _, sqs = base.shaped(ho.COSINE, 20, "dense")
    metric, gm = NINE[0], base.g_metric(NINE[0])
    ip, pos, val = mo.csr_of([sqs[0], sqs[1], sqs[0]])
    ip = ip.astype(np.int64)
    pos = pos.copy()
    pos[ip[1]] = 20                                  # query 1: a position == dim
    ip[3] += 5                                       # query 2: past nnz_total
    got = host4(g.cache_search_sparse_device(*dev_csr((ip, pos, val)), 4, 0.2, gm))
    assert got[3].tolist() == [0, 1, 2]
    assert not got[2][1:].any() and (got[0][1:] == NONE64).all() and np.isneginf(got[1][1:]).all()
    base.assert_answers(metric, tuple(a[:1] for a in got[:3]),
                        [co.search_nodes_sparse(o, lambda n: bool(live[n]), sqs[0], 4, 0.2, metric)], 4, "beside statuses")

    rows = np.random.default_rng(4).standard_normal((12, 8)).astype(F)
    csr = (np.array([0, 2], np.uint64), np.array([1, 5], np.uint32), np.array([1.0, -2.0], F))

    def refused(h, word):
        out = (torch.full((1, 3), 77, dtype=torch.int64, device="cuda"), torch.full((1, 3), 7.0, dtype=torch.float32, device="cuda"),
               torch.full((1,), 99, dtype=torch.int32, device="cuda"))
        with pytest.raises(NeumannGpuError) as e:
            h.cache_search_sparse_device(*dev_csr(csr), 3, 0.0, ExtendedDistanceMetric.Cosine, out=out)
        assert e.value.status == _capi.ERR_CONFIGURATION and word in str(e.value), str(e.value)
        torch.cuda.synchronize()
        assert (out[0] == 77).all() and (out[1] == 7.0).all() and (out[2] == 99).all()

    with GpuHnsw(8, base.g_config(ho.HNSWConfig(**base.SMALL)), storage="quantized") as h:
        h.insert(rows)
        refused(h, "quantized")
    with GpuHnsw(8, base.g_config(ho.HNSWConfig(**base.SMALL).with_distance_metric(ho.EUCLIDEAN))) as h:
        h.insert(rows)
        h.insert_sparse([0, 2], [1, 4], [1.0, 2.0])
        refused(h, "Euclidean")
