"""tests/_hnsw_tt_oracle.py against hand-derived values, the library's host restatement of the same loops against the twin, the
new symbols, and the frozen fixture tests/golden/hnsw_tt_small.npz (docs/hnsw.md §17).  No GPU."""
import ctypes as C
import math
import os
import re
from fractions import Fraction

import numpy as np
import pytest

from tests import _hnsw_mixed_oracle as mo
from tests import _hnsw_oracle as ho
from tests import _hnsw_q8_oracle as qo
from tests import _hnsw_tt_oracle as to

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "hnsw_tt_small.npz")


def bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


def test_one_core_norm_is_a_sequential_chain_not_simd_magnitude():
    """[4096, 1, 1, ...]: the Gram chain adds 1.0 to 2^24 fifteen times and stays at 2^24 (ties to even): the norm is 4096.0 exactly.
    simd::magnitude of the reconstruction keeps eight chains: 2^24 + 1 -> 2^24 in chain 0, 1 + 1 in the seven others, 2^24 + 14."""
    v = np.ones(16, dtype=F)
    v[0] = 4096.0
    tt = to.TTVector([16], [1, 1], [v])
    recon = to.tt_reconstruct(tt)
    assert np.array_equal(bits(recon), bits(v))
    assert bits(to.tt_norm(tt)) == 0x45800000                      # 4096.0
    mag = ho.magnitude(recon)
    assert bits(mag) == 0x45800003                                 # 4096 + 3 * 2^-11
    c, half = Fraction(4096) + Fraction(3, 2048), Fraction(1, 4096)  # the correctly rounded sqrt(2^24 + 14), checked exactly
    assert (c - half) ** 2 < 2 ** 24 + 14 < (c + half) ** 2


def two_core_train():
    g1 = np.array([[[1, 2], [3, 4]]], dtype=F)          # [1][2][2]: G1[0, j, r]
    g2 = np.array([[[5], [6]], [[7], [8]]], dtype=F)    # [2][2][1]: G2[l, j, 0]
    return to.TTVector([2, 2], [1, 2, 1], [g1, g2])


def test_two_core_train_by_hand():
    """element (i0, i1) = G1[0,i0,0] G2[0,i1,0] + G1[0,i0,1] G2[1,i1,0]: 19, 22, 43, 50.  Gram after core 1: [[10, 14], [14, 20]];
    after core 2: k = 0 gives 10 25 + 14 35 + 14 35 + 20 49 = 2210, k = 1 gives 360 + 672 + 672 + 1280 = 2984: 5194 = |v|^2."""
    tt = two_core_train()
    assert to.tt_reconstruct(tt).tolist() == [19.0, 22.0, 43.0, 50.0]
    assert 19 ** 2 + 22 ** 2 + 43 ** 2 + 50 ** 2 == 5194
    assert bits(to.tt_norm(tt)) == bits(np.sqrt(F(5194.0)))
    assert abs(float(to.tt_norm(tt)) - math.sqrt(5194.0)) < 4e-6
    shape, ranks, off, cores = to.pack([tt])
    assert cores.tolist() == [1, 2, 3, 4, 5, 6, 7, 8] and off.tolist() == [0, 8] and ranks.tolist() == [[1, 2, 1]]


def single(x, shape=(2, 2, 5)):
    """a rank-one train whose reconstruction is x at element 0 and zeros elsewhere"""
    cores = [np.zeros(n, dtype=F) for n in shape]
    for c in cores:
        c[0] = 1.0
    cores[0][0] = x
    return to.TTVector(list(shape), [1] * (len(shape) + 1), cores)


def test_the_norm_threshold_zero_and_nan():
    tiny = F(1e-10)
    below, above = np.nextafter(tiny, F(0)), np.nextafter(tiny, F(1))
    norms = [to.tt_norm(single(x)) for x in (below, tiny, above)]
    assert [bits(n).item() for n in norms] == [bits(x).item() for x in (below, tiny, above)]   # sqrt(x * x) == x here
    rows = np.random.default_rng(3).standard_normal((30, 20)).astype(F)
    rows[7] = 0.0
    idx = ho.build(rows, ho.HNSWConfig.high_speed())
    ids = list(range(30))
    d_below = to.cosine_distance_tt_with_norm(idx, ids, to.tt_reconstruct(single(below)), norms[0])
    assert (d_below == 1.0).all()                                                          # query_norm < 1e-10
    for x, n in ((tiny, norms[1]), (above, norms[2])):                                     # not below: the arithmetic runs
        q = to.tt_reconstruct(single(x))
        d = to.cosine_distance_tt_with_norm(idx, ids, q, n)
        with np.errstate(all="ignore"):
            want = F(1.0) - (rows[:, 0] * x) / (idx.mags[:30] * n)
        want[7] = 1.0                                                                      # mag_self == 0.0
        assert np.array_equal(bits(d), bits(want))
        assert (d != 1.0).sum() >= 28
    zero = to.TTVector([2, 2, 5], [1, 2, 2, 1], [np.zeros(4), np.zeros(8), np.zeros(10)])
    assert bits(to.tt_norm(zero)) == 0 and not to.tt_reconstruct(zero).any()
    assert (to.cosine_distance_tt_with_norm(idx, ids, to.tt_reconstruct(zero), to.tt_norm(zero)) == 1.0).all()
    assert [s for _, s in to.search_tt_with_ef(idx, zero, 5, 20)] == [0.0] * 5
    nan = to.random_tt(np.random.default_rng(4), [2, 2, 5], [1, 2, 2, 1])
    nan.cores[1][1, 0, 1] = np.nan
    assert np.isnan(to.tt_norm(nan)) and np.isnan(to.tt_reconstruct(nan)).any()
    d = to.cosine_distance_tt_with_norm(idx, ids, to.tt_reconstruct(nan), to.tt_norm(nan))
    assert np.isnan(np.delete(d, 7)).all() and d[7] == 1.0                                 # NaN < 1e-10 is false


@pytest.mark.parametrize("shape,ranks", [([1, 5], [1, 3, 1]), ([3, 1, 5], [1, 2, 2, 1]), ([1, 1, 7], [1, 1, 1, 1]), ([2, 2, 5], [1, 2, 2, 1]),
                                         ([2] * 6, [1, 2, 4, 3, 2, 2, 1])])
def test_shapes_with_a_mode_of_one_against_exact_integers(shape, ranks):
    """small integer cores: every product and sum is exact, so the chains must give the contraction computed in integers"""
    rng = np.random.default_rng(len(shape) * 100 + sum(ranks))
    tt = to.TTVector(shape, ranks, [rng.integers(-3, 4, (ranks[k], shape[k], ranks[k + 1])) for k in range(len(shape))])
    full = tt.cores[0].astype(np.int64)[0]                       # [n_1][r_1]
    for c in tt.cores[1:]:
        full = np.tensordot(full, c.astype(np.int64), axes=([full.ndim - 1], [0]))
    want = full.reshape(-1)
    assert to.tt_reconstruct(tt).tolist() == want.tolist()
    assert bits(to.tt_norm(tt)) == bits(np.sqrt(F(int((want * want).sum()))))


def test_distance_on_sparse_and_quantized_nodes():
    """dot_with_tt reconstructs the query, then dot_dense of the node's own kind; magnitude() is the node's own"""
    rng = np.random.default_rng(12)
    rows = rng.standard_normal((40, 20)).astype(F)
    mask = np.arange(40) % 2 == 1
    rows[mask] = mo.sparsify(rng, rows[mask], 0.6)
    tt = to.random_tt(rng, [2, 2, 5], [1, 2, 2, 1])
    q, n = to.tt_reconstruct(tt), to.tt_norm(tt)
    mixed = mo.build_mixed(rows, mask, ho.HNSWConfig.high_speed().with_distance_metric(ho.EUCLIDEAN))
    d = to.cosine_distance_tt_with_norm(mixed, range(40), q, n)
    for i in range(40):
        if mask[i]:
            s = mixed.sparse[i]
            want = F(1.0) - F(s.dot_dense(q)) / (F(s.magnitude()) * n)
        else:
            want = F(1.0) - ho.dot_product_rows(rows[i:i + 1], q)[0] / (ho.magnitude(rows[i]) * n)
        assert bits(d[i]) == bits(want), i
    q8 = qo.build(rows, ho.HNSWConfig.high_speed().with_distance_metric(ho.DOT_PRODUCT))
    d = to.cosine_distance_tt_with_norm(q8, range(40), q, n)
    for i in range(40):
        dot = qo.dot_dense(q8.codes[i], q8.scale[i], q8.min_val[i], q)[0]
        assert bits(d[i]) == bits(F(1.0) - dot / (ho.magnitude(q8.get_vector(i)) * n)), i


def test_host_restatement_equals_the_twin():
    """NMN_HNSW_HOST_SEARCH=1 sends every train to the library's host loops (what a train above the LDS limits takes): no GPU needed"""
    from neumann_amd import TTVector, tt, tt_norm, tt_reconstruct
    assert tt.limits()[:3] == (8, 32, 8192)
    rng = np.random.default_rng(77)
    old = os.environ.get("NMN_HNSW_HOST_SEARCH")
    os.environ["NMN_HNSW_HOST_SEARCH"] = "1"
    try:
        for shape, ranks in (([2, 2, 5], [1, 2, 2, 1]), ([7], [1, 1]), ([1, 5], [1, 3, 1]), ([4, 4, 8], [1, 4, 2, 1]),
                             ([2] * 6, [1, 2, 4, 3, 2, 2, 1]), ([2, 3, 2], [1, 33, 33, 1])):
            ts = [to.random_tt(rng, shape, ranks) for _ in range(3)]
            lts = [TTVector(t.shape, t.ranks, t.cores) for t in ts]
            assert np.array_equal(bits(tt_reconstruct(lts)), bits(np.stack([to.tt_reconstruct(t) for t in ts])))
            assert np.array_equal(bits(tt_norm(lts)), bits(np.asarray([to.tt_norm(t) for t in ts], dtype=F)))
    finally:
        if old is None:
            del os.environ["NMN_HNSW_HOST_SEARCH"]
        else:
            os.environ["NMN_HNSW_HOST_SEARCH"] = old


def test_malformed_trains_are_refused_before_anything_runs():
    from neumann_amd import _capi
    lib = _capi.load()
    p = lambda a: C.c_void_p(a.ctypes.data)   # noqa: E731

    def norm(shape, ranks, off, cores, nq):
        shape, ranks = np.asarray(shape, dtype=np.uint32), np.asarray(ranks, dtype=np.uint32)
        off, cores = np.asarray(off, dtype=np.uint64), np.asarray(cores, dtype=F)
        out = np.full(nq, 7, dtype=F)
        st = lib.nmn_tt_norm(p(shape), shape.size, p(ranks), p(off), p(cores), nq, p(out))
        assert (out == 7).all()
        return st, lib.nmn_last_error().decode()

    z = np.zeros(64)
    assert norm([2, 2], [[1, 2, 1], [2, 2, 1]], [0, 8, 16], z, 2)[0] == _capi.ERR_INVALID_ARGUMENT
    st, text = norm([2, 2], [[1, 2, 1], [1, 2, 2]], [0, 8, 16], z, 2)
    assert st == _capi.ERR_INVALID_ARGUMENT and "query 1" in text and "ranks[0] and ranks[n_cores] must be 1" in text
    st, text = norm([2, 2], [[1, 2, 1], [1, 0, 1]], [0, 8, 8], z, 2)
    assert st == _capi.ERR_INVALID_ARGUMENT and "query 1" in text and "rank" in text
    st, text = norm([2, 2], [[1, 2, 1]], [0, 9], z, 1)
    assert st == _capi.ERR_INVALID_ARGUMENT and "query 0" in text and "core_off" in text
    assert norm([2, 0], [[1, 2, 1]], [0, 8], z, 1)[0] == _capi.ERR_INVALID_ARGUMENT
    assert norm([], np.ones((1, 1)), [0, 0], z, 1)[0] == _capi.ERR_INVALID_ARGUMENT
    assert norm([2] * 9, np.ones((1, 10)), [0, 18], z, 1)[0] == _capi.ERR_INVALID_ARGUMENT


def test_new_symbols_are_exported_declared_and_bound():
    from neumann_amd import GpuHnsw, _capi
    lib = _capi.load()
    header = open(os.path.join(ROOT, "include", "neumann_gpu.h")).read()
    ffi = open(os.path.join(ROOT, "integration", "rust", "ffi.rs")).read()
    wrapper = open(os.path.join(ROOT, "integration", "rust", "gpu_index.rs")).read()
    for name in ("nmn_tt_reconstruct", "nmn_tt_norm", "nmn_tt_limits", "nmn_hnsw_search_tt", "nmn_hnsw_search_tt_device",
                 "nmn_hnsw_insert_tt"):
        assert hasattr(lib, name), name
        assert re.search(rf"\b{name}\s*\(", header), name
        assert name in _capi.SIGNATURES, name
        assert re.search(rf"pub fn {name}\(", ffi), name
    for m in ("search_tt", "insert_tt"):
        assert f"pub fn {m}(" in wrapper and f"ffi::nmn_hnsw_{m}(" in wrapper, m
    for m in ("search_tt", "search_tt_device", "insert_tt"):
        assert callable(getattr(GpuHnsw, m))


def test_golden_fixture_is_the_twin_and_not_densification():
    z = np.load(GOLDEN)
    tts = to.golden_trains()
    shape, ranks, off, cores = to.pack(tts)
    assert shape.tolist() == [2, 2, 5] and np.array_equal(z["ranks"], ranks) and np.array_equal(z["core_off"], off)
    assert np.array_equal(bits(z["cores"]), bits(cores))
    assert np.array_equal(bits(z["reconstructions"]), bits(np.stack([to.tt_reconstruct(t) for t in tts])))
    assert np.array_equal(bits(z["norms"]), bits(np.asarray([to.tt_norm(t) for t in tts], dtype=F)))
    # what the fixture script counted, pinned: answers whose ids or score bits differ from `search` of the reconstructed query
    assert int(z["norms_differ"]) == 33
    assert int(z["cosine_differ"]) == 33 and int(z["cosine_differ"]) >= 8
    assert int(z["euclidean_differ"]) == 64 and int(z["dot_differ"]) == 64
    rows, _ = ho.golden_corpus()
    idx = ho.build(rows[:800], ho.HNSWConfig().with_distance_metric(ho.EUCLIDEAN))
    ids, sc, cnt = to.answers_tt(idx, tts[:16], 10, 50)
    assert np.array_equal(ids, z["euclidean_ids"][:16]) and np.array_equal(bits(sc), bits(z["euclidean_scores"][:16]))
    assert np.array_equal(cnt, z["euclidean_counts"][:16])
    dids, dsc, _ = ho.padded_answers(idx, z["reconstructions"][:16], 10, 50)
    assert ((ids != dids) | (bits(sc) != bits(dsc))).any(axis=1).all()
