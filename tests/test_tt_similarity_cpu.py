"""tests/_tt_similarity_oracle.py against hand-derived values, the library's host restatement of the same loops against the twin, every
refusal, the new symbols, and the frozen fixture tests/golden/tt_similarity_small.npz (docs/hnsw.md §23).  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import _hnsw_oracle as ho
from tests import _hnsw_tt_oracle as to
from tests import _tt_similarity_oracle as so

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "tt_similarity_small.npz")
NAN_BITS = 0x7FC00000


def bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


def same(got, want):
    """bit for bit, a NaN compared as a NaN"""
    got, want = np.asarray(got, dtype=F), np.asarray(want, dtype=F)
    return got.shape == want.shape and bool(((bits(got) == bits(want)) | (np.isnan(got) & np.isnan(want))).all())


class host_only:
    """NMN_HNSW_HOST_SEARCH=1: every pair goes to the library's host restatement — no GPU needed"""

    def __enter__(self):
        self.old = os.environ.get("NMN_HNSW_HOST_SEARCH")
        os.environ["NMN_HNSW_HOST_SEARCH"] = "1"

    def __exit__(self, *exc):
        if self.old is None:
            del os.environ["NMN_HNSW_HOST_SEARCH"]
        else:
            os.environ["NMN_HNSW_HOST_SEARCH"] = self.old


def lib_trains(ts):
    from neumann_amd import TTVector
    return [TTVector(t.shape, t.ranks, t.cores) for t in ts]


def one_core(values):
    return so.TTVector([len(values)], [1, 1], [np.asarray(values, dtype=F)])


def test_one_core_dot_is_one_sequential_chain_in_k():
    """2^24 + 1 is 2^24 (the tie goes to even), then - 2^24: 0.0; in the other order 2^24 - 2^24 + 1: 1.0"""
    ones = one_core([1, 1, 1])
    assert bits(so.tt_dot_product(one_core([2.0 ** 24, 1, -2.0 ** 24]), ones)) == bits(F(0.0))
    assert bits(so.tt_dot_product(one_core([2.0 ** 24, -2.0 ** 24, 1]), ones)) == bits(F(1.0))


def two_core_pair():
    a = so.TTVector([2, 2], [1, 2, 1], [np.array([[[1, 2], [3, 4]]], dtype=F), np.array([[[5], [6]], [[7], [8]]], dtype=F)])
    b = so.TTVector([2, 2], [1, 3, 1], [np.array([[[1, 2, 3], [4, 5, 6]]], dtype=F),
                                        np.array([[[1], [2]], [[3], [4]], [[5], [6]]], dtype=F)])
    return a, b


def test_two_core_pair_of_different_ranks_by_hand():
    """Gram after core 1, [x][y] = A1[0,0,x] B1[0,0,y] + A1[0,1,x] B1[0,1,y]: [[13, 17, 21], [18, 24, 30]].  After core 2: k = 0 gives
    5 (13 1 + 17 3 + 21 5) + 7 (18 1 + 24 3 + 30 5) = 845 + 1680, k = 1 gives 6 (26 + 68 + 126) + 8 (36 + 96 + 180) = 1320 + 2496:
    6341.  The dense vectors are [19, 22, 43, 50] and [22, 28, 49, 64]: 418 + 616 + 2107 + 3200 = 6341."""
    a, b = two_core_pair()
    gram1 = np.einsum("kx,ky->xy", a.cores[0][0].astype(np.int64), b.cores[0][0].astype(np.int64))
    assert gram1.tolist() == [[13, 17, 21], [18, 24, 30]]
    assert so.tt_dot_product(a, b) == 6341.0 and so.tt_dot_product(b, a) == 6341.0
    assert to.tt_reconstruct(a).tolist() == [19, 22, 43, 50] and to.tt_reconstruct(b).tolist() == [22, 28, 49, 64]
    assert so.self_dot(a) == 5194.0 and bits(np.sqrt(so.self_dot(a))) == bits(to.tt_norm(a))
    # every step of the chain of new_gram[0] after core 1, restated term by term: k, then ia, then ib
    chain = F(0.0)
    for k in range(2):
        for ia in range(1):
            for ib in range(1):
                chain = F(chain + F(F(F(1.0) * a.cores[0][ia, k, 0]) * b.cores[0][ib, k, 0]))
    assert chain == 13.0


def test_the_dot_is_not_symmetric_in_bits_and_not_the_dense_dot():
    qs, ts = so.golden_sets()
    pairs = [(q, t) for q in qs[:4] for t in ts[:6]]
    swapped = [(q, t) for q, t in pairs if bits(so.tt_dot_product(q, t)) != bits(so.tt_dot_product(t, q))]
    assert len(swapped) >= 6, len(swapped)                 # the products are (g * A) * B
    q, t = swapped[0]
    dense = ho.dot_product_rows(to.tt_reconstruct(t)[None, :], to.tt_reconstruct(q))[0]
    assert abs(float(so.tt_dot_product(q, t)) - float(dense)) <= 1e-4 * max(1.0, abs(float(dense)))


def single(x, shape=(2, 2, 5)):
    """a rank-one train whose reconstruction is x at element 0 and zeros elsewhere: its self dot is x * x"""
    cores = [np.zeros(n, dtype=F) for n in shape]
    for c in cores:
        c[0] = 1.0
    cores[0][0] = x
    return so.TTVector(list(shape), [1] * (len(shape) + 1), cores)


def special_pairs():
    """(name, a, b): the trains whose comparison leaves the ordinary arithmetic"""
    tiny = F(1e-10)
    below, above = np.nextafter(tiny, F(0)), np.nextafter(tiny, F(1))
    one = single(F(1.0))
    zero = so.TTVector([2, 2, 5], [1, 2, 2, 1], [np.zeros(4), np.zeros(8), np.zeros(10)])
    nan = so.random_tt(np.random.default_rng(4), [2, 2, 5], [1, 2, 2, 1])
    nan.cores[1][1, 0, 1] = np.nan
    plain = so.random_tt(np.random.default_rng(5), [2, 2, 5], [1, 2, 2, 1])
    z = np.load(GOLDEN)
    neg_a = so.TTVector([2, 2, 5], z["neg_ranks"][0], np.split(z["neg_cores_a"], [4, 12]))
    neg_b = so.TTVector([2, 2, 5], z["neg_ranks"][0], np.split(z["neg_cores_b"], [4, 12]))
    return [("below", single(below), one), ("at", single(tiny), one), ("above", single(above), one), ("below_b", one, single(below)),
            ("zero_zero", zero, zero), ("zero_plain", zero, plain), ("nan_plain", nan, plain), ("plain_nan", plain, nan),
            ("nan_nan", nan, nan), ("negative_sq", neg_a, neg_b)]


def test_cosine_threshold_zero_nan_and_the_clamp():
    by = {name: (a, b) for name, a, b in special_pairs()}
    tiny = F(1e-10)
    for name, x in (("below", np.nextafter(tiny, F(0))), ("at", tiny), ("above", np.nextafter(tiny, F(1)))):
        a, b = by[name]
        assert bits(np.sqrt(so.self_dot(a))) == bits(x)                           # sqrt(x * x) == x here
        assert bits(so.tt_dot_product(a, b)) == bits(x)
        assert bits(so.tt_cosine_similarity(a, b)) == bits(F(0.0) if name == "below" else F(1.0)), name   # norm_a < 1e-10
    assert bits(so.tt_cosine_similarity(*by["below_b"])) == 0                      # norm_b < 1e-10
    zero, plain = by["zero_plain"]
    assert bits(so.tt_dot_product(zero, plain)) == 0 and bits(so.tt_dot_product(zero, zero)) == 0    # +0.0, never -0.0
    assert bits(so.tt_cosine_similarity(zero, plain)) == 0 and bits(so.tt_euclidean_distance(zero, zero)) == 0
    assert bits(so.tt_euclidean_distance(zero, plain)) == bits(np.sqrt(so.self_dot(plain)))
    nan, _ = by["nan_plain"]
    for a, b in (by["nan_plain"], by["plain_nan"], by["nan_nan"]):
        assert np.isnan(so.tt_dot_product(a, b)) and np.isnan(so.tt_cosine_similarity(a, b))        # NaN < 1e-10 is false
        assert bits(so.tt_euclidean_distance(a, b)) == 0                                             # NaN.max(0.0) is 0.0
    assert np.isnan(so.self_dot(nan))
    a, b = by["negative_sq"]
    z = np.load(GOLDEN)
    sq = so.qo.fma32(F(-2.0), so.tt_dot_product(a, b), so.self_dot(a) + so.self_dot(b))
    assert sq < 0 and bits(sq) == bits(z["neg_sq"]) and int(z["neg_count"]) >= 1
    assert bits(so.tt_euclidean_distance(a, b)) == 0
    assert not np.array_equal(bits(a.flat()), bits(b.flat()))


def test_batch_forms_fail_as_a_whole():
    from neumann_amd import NeumannGpuError, tt_cosine_similarity_batch, tt_dot_product_batch, tt_euclidean_distance_batch
    rng = np.random.default_rng(9)
    q = so.random_tt(rng, [2, 2, 5], [1, 2, 2, 1])
    ts = [so.random_tt(rng, [2, 2, 5], [1, 2, 2, 1]) for _ in range(5)]
    odd = so.random_tt(rng, [2, 5, 2], [1, 2, 2, 1])
    for op in (so.DOT, so.COSINE, so.EUCLIDEAN):
        with pytest.raises(so.TTError, match=so.INCOMPATIBLE_SHAPES):
            so.batch(op, q, ts[:3] + [odd] + ts[3:])
    with host_only():
        lq, lts, lodd = lib_trains([q])[0], lib_trains(ts), lib_trains([odd])[0]
        for fn, op in ((tt_dot_product_batch, so.DOT), (tt_cosine_similarity_batch, so.COSINE), (tt_euclidean_distance_batch, so.EUCLIDEAN)):
            assert same(fn(lq, lts), so.batch(op, q, ts))
            assert same(fn(lq, lts[:3]), so.batch(op, q, ts[:3]))          # below the rayon split at 4: the same values
            with pytest.raises(NeumannGpuError, match=so.INCOMPATIBLE_SHAPES):
                fn(lq, lts[:3] + [lodd] + lts[3:])
            assert fn(lq, []).shape == (0,)


HOST_CASES = [([2, 2, 5], [1, 2, 2, 1], [1, 2, 3, 1]), ([7], [1, 1], [1, 1]), ([1, 5], [1, 3, 1], [1, 2, 1]), ([4, 4, 8], [1, 4, 2, 1], [1, 3, 5, 1]),
              ([2] * 6, [1, 2, 4, 3, 2, 2, 1], [1, 2, 2, 2, 2, 2, 1]), ([2, 3, 2], [1, 33, 33, 1], [1, 2, 34, 1]), ([3, 1, 5], [1, 2, 2, 1], [1, 1, 1, 1])]


@pytest.mark.parametrize("shape,ranks_q,ranks_t", HOST_CASES)
def test_host_restatement_equals_the_twin(shape, ranks_q, ranks_t):
    from neumann_amd import tt, tt_norm
    rng = np.random.default_rng(len(shape) * 1000 + sum(ranks_q) * 10 + sum(ranks_t))
    qs = [so.random_tt(rng, shape, ranks_q) for _ in range(3)]
    ts = [so.random_tt(rng, shape, ranks_t if j % 2 else ranks_q) for j in range(5)]
    with host_only():
        lq, lt = lib_trains(qs), lib_trains(ts)
        for op in (so.DOT, so.COSINE, so.EUCLIDEAN):
            assert same(tt.tt_similarity(op, lq, lt), so.similarity(op, qs, ts)), op
        selfs = tt.tt_self_dot(lt)
        assert same(selfs, [so.self_dot(t) for t in ts])
        assert same(np.sqrt(selfs), tt_norm(lt))                        # the chain tt_norm runs before its square root
        assert same(tt.tt_dot_product(lq[0], lt[1]), so.tt_dot_product(qs[0], ts[1]))
        assert same(tt.tt_cosine_similarity(lq[0], lt[1]), so.tt_cosine_similarity(qs[0], ts[1]))
        assert same(tt.tt_euclidean_distance(lq[0], lt[1]), so.tt_euclidean_distance(qs[0], ts[1]))


def test_a_call_with_no_pair_for_the_kernel_is_the_hosts():
    """every query above the limits (rank 33): no pair is left for the device, so none is touched — and the self dots of the
    targets, which the kernel could have taken, are the host's as well"""
    from neumann_amd import tt
    rng = np.random.default_rng(33)
    qs = [so.random_tt(rng, [2, 3, 2], [1, 33, 33, 1]) for _ in range(2)]
    ts = [so.random_tt(rng, [2, 3, 2], [1, 3, 2, 1]) for _ in range(3)]
    for op in (so.DOT, so.COSINE, so.EUCLIDEAN):
        assert same(tt.tt_similarity(op, lib_trains(qs), lib_trains(ts)), so.similarity(op, qs, ts)), op
        assert same(tt.tt_similarity(op, lib_trains(ts), lib_trains(qs)), so.similarity(op, ts, qs)), op
    assert same(tt.tt_self_dot(lib_trains(qs)), [so.self_dot(q) for q in qs])


def test_host_restatement_on_the_special_trains_and_in_threads():
    from neumann_amd import tt
    sp = special_pairs()
    a, b = [p[1] for p in sp], [p[2] for p in sp]
    with host_only():
        for op in (so.DOT, so.COSINE, so.EUCLIDEAN):
            want = so.similarity(op, a, b)
            assert same(tt.tt_similarity(op, lib_trains(a), lib_trains(b)), want), op
            os.environ["NMN_TT_SIMILARITY_HOST_THREADS"] = "1"
            try:
                assert same(tt.tt_similarity(op, lib_trains(a), lib_trains(b)), want), op
            finally:
                del os.environ["NMN_TT_SIMILARITY_HOST_THREADS"]


def p(a):
    return C.c_void_p(a.ctypes.data)


def test_every_refusal_leaves_the_outputs_untouched():
    from neumann_amd import _capi
    lib = _capi.load()

    def sim(op, q, t, nq=None, nt=None, out_null=False):
        """q, t: (shape, ranks, core_off, cores)"""
        arrs = []
        for shape, ranks, off, cores in (q, t):
            arrs.append((np.asarray(shape, dtype=np.uint32), np.asarray(ranks, dtype=np.uint32), np.asarray(off, dtype=np.uint64),
                         np.asarray(cores, dtype=F)))
        nq = arrs[0][1].shape[0] if nq is None else nq
        nt = arrs[1][1].shape[0] if nt is None else nt
        out = np.full((max(nq, 1), max(nt, 1)), 7, dtype=F)
        (sq, rq, oq, cq), (st, rt, ot, ct) = arrs
        code = lib.nmn_tt_similarity(op, p(sq), sq.size, p(rq), p(oq), p(cq), nq, p(st), st.size, p(rt), p(ot), p(ct), nt,
                                     None if out_null else p(out))
        assert (out == 7).all()
        return code, lib.nmn_last_error().decode()

    z = np.zeros(64)
    good = ([2, 2], [[1, 2, 1], [1, 2, 1]], [0, 8, 16], z)
    bad_end = ([2, 2], [[1, 2, 1], [1, 2, 2]], [0, 8, 16], z)
    code, text = sim(3, good, good)
    assert code == _capi.ERR_INVALID_ARGUMENT and "unknown op" in text
    code, text = sim(0, bad_end, good)
    assert code == _capi.ERR_INVALID_ARGUMENT and "query set" in text and "train 1" in text and "ranks[0] and ranks[n_cores] must be 1" in text
    code, text = sim(0, good, bad_end)
    assert code == _capi.ERR_INVALID_ARGUMENT and "target set" in text and "train 1" in text
    code, text = sim(1, good, ([2, 2], [[1, 2, 1], [1, 0, 1]], [0, 8, 8], z))
    assert code == _capi.ERR_INVALID_ARGUMENT and "target set" in text and "train 1" in text and "rank" in text
    code, text = sim(2, ([2, 2], [[1, 2, 1]], [0, 9], z), good)
    assert code == _capi.ERR_INVALID_ARGUMENT and "query set" in text and "train 0" in text and "core_off" in text
    code, text = sim(0, good, ([2, 0], [[1, 2, 1]], [0, 8], z))
    assert code == _capi.ERR_INVALID_ARGUMENT and "target set" in text
    code, text = sim(0, good, ([2] * 9, np.ones((1, 10)), [0, 18], z))
    assert code == _capi.ERR_INVALID_ARGUMENT and "target set" in text and "n_cores" in text
    for other in (([2, 3], [[1, 2, 1]], [0, 10], z), ([2, 2, 1], [[1, 2, 1, 1]], [0, 9], z), ([4], [[1, 1]], [0, 4], z)):
        for op in (0, 1, 2):
            code, text = sim(op, good, other)                            # IncompatibleShapes: a mode, or the number of modes
            assert code == _capi.ERR_INVALID_ARGUMENT and text == so.INCOMPATIBLE_SHAPES
            code, text = sim(op, other, good)
            assert code == _capi.ERR_INVALID_ARGUMENT and text == so.INCOMPATIBLE_SHAPES
    assert sim(0, good, good, out_null=True)[0] == _capi.ERR_INVALID_ARGUMENT
    assert sim(0, good, good, nq=0)[0] == _capi.OK and sim(2, good, good, nt=0)[0] == _capi.OK      # nothing to do, nothing written
    # nmn_tt_self_dot
    sh, rk, off = np.asarray([2, 2], dtype=np.uint32), np.asarray([[1, 2, 1], [1, 2, 2]], dtype=np.uint32), np.asarray([0, 8, 16], dtype=np.uint64)
    cores, out = np.zeros(64, dtype=F), np.full(2, 7, dtype=F)
    assert lib.nmn_tt_self_dot(p(sh), 2, p(rk), p(off), p(cores), 2, p(out)) == _capi.ERR_INVALID_ARGUMENT
    assert "train 1" in lib.nmn_last_error().decode() and (out == 7).all()
    assert lib.nmn_tt_self_dot(p(sh), 2, p(rk), p(off), p(cores), 0, p(out)) == _capi.OK and (out == 7).all()
    # the device entries refuse what the host can see before anything is enqueued (the pointers are never read)
    rk[1] = [1, 2, 1]
    fake = p(cores)

    def dev(op=0, n_cores=2, stride_q=8, stride_t=8, self_q=fake, self_t=fake, shape=sh):
        return lib.nmn_tt_similarity_device(op, p(shape), n_cores, p(rk), None, fake, stride_q, None, 2, p(rk), None, fake, stride_t, None, 2,
                                            self_q, self_t, p(out), None)
    assert dev(op=3) == _capi.ERR_INVALID_ARGUMENT and "unknown op" in lib.nmn_last_error().decode()
    assert dev(n_cores=9) == _capi.ERR_INVALID_ARGUMENT and dev(n_cores=0) == _capi.ERR_INVALID_ARGUMENT
    assert dev(stride_q=0) == _capi.ERR_INVALID_ARGUMENT and "query set" in lib.nmn_last_error().decode()
    assert dev(stride_t=8193) == _capi.ERR_INVALID_ARGUMENT and "target set" in lib.nmn_last_error().decode()
    assert dev(op=1, self_q=None) == _capi.ERR_INVALID_ARGUMENT and dev(op=2, self_t=None) == _capi.ERR_INVALID_ARGUMENT
    assert dev(shape=np.asarray([2, 0], dtype=np.uint32)) == _capi.ERR_INVALID_ARGUMENT
    assert lib.nmn_tt_self_dot_device(p(sh), 2, p(rk), None, fake, 8193, None, 2, p(out), None) == _capi.ERR_INVALID_ARGUMENT
    assert lib.nmn_tt_self_dot_device(p(sh), 9, p(rk), None, fake, 8, None, 2, p(out), None) == _capi.ERR_INVALID_ARGUMENT
    assert lib.nmn_tt_self_dot_device(p(sh), 2, None, None, fake, 8, None, 2, p(out), None) == _capi.ERR_INVALID_ARGUMENT
    assert (out == 7).all()


def test_new_symbols_are_exported_declared_and_bound():
    import neumann_amd
    from neumann_amd import _capi, tt
    lib = _capi.load()
    header = open(os.path.join(ROOT, "include", "neumann_gpu.h")).read()
    ffi = open(os.path.join(ROOT, "integration", "rust", "ffi.rs")).read()
    for name in ("nmn_tt_similarity", "nmn_tt_self_dot", "nmn_tt_self_dot_device", "nmn_tt_similarity_device"):
        assert hasattr(lib, name), name
        assert re.search(rf"\b{name}\s*\(", header), name
        assert name in _capi.SIGNATURES, name
        assert re.search(rf"pub fn {name}\(", ffi), name
    for macro, value in (("NMN_TT_SIM_DOT", 0), ("NMN_TT_SIM_COSINE", 1), ("NMN_TT_SIM_EUCLIDEAN", 2)):
        assert re.search(rf"#define {macro} {value}u", header), macro
    for fn in ("tt_dot_product", "tt_cosine_similarity", "tt_euclidean_distance", "tt_dot_product_batch", "tt_cosine_similarity_batch",
               "tt_euclidean_distance_batch", "tt_similarity", "tt_self_dot", "tt_similarity_device"):
        assert callable(getattr(tt, fn)) and callable(getattr(neumann_amd, fn)), fn
    assert (tt.SIM_DOT, tt.SIM_COSINE, tt.SIM_EUCLIDEAN) == (so.DOT, so.COSINE, so.EUCLIDEAN)


def test_golden_fixture_is_the_twin_and_not_reconstruction():
    from neumann_amd import tt
    z = np.load(GOLDEN)
    qs, ts = so.golden_sets()
    shape, rq, oq, cq = so.pack(qs)
    _, rt, ot, ct = so.pack(ts)
    assert shape.tolist() == [2, 2, 5] and np.array_equal(z["ranks_q"], rq) and np.array_equal(z["ranks_t"], rt)
    assert (rq == [1, 2, 2, 1]).all() and (rt[1::2] == [1, 2, 3, 1]).all() and (rt[0::2] == [1, 2, 2, 1]).all()
    assert np.array_equal(z["core_off_q"], oq) and np.array_equal(z["core_off_t"], ot)
    assert np.array_equal(bits(z["cores_q"]), bits(cq)) and np.array_equal(bits(z["cores_t"]), bits(ct))
    for name, op in (("dot", so.DOT), ("cosine", so.COSINE), ("euclidean", so.EUCLIDEAN)):
        assert z[name].shape == (16, 24) and same(z[name], so.similarity(op, qs, ts)), name
    # what the fixture script counted, pinned
    assert int(z["dense_differ"]) == 319 and int(z["dense_differ"]) >= 192
    assert int(z["swapped_differ"]) == 313 and int(z["swapped_differ"]) >= 96
    rec_t = np.stack([to.tt_reconstruct(t) for t in ts])
    dense = np.stack([ho.dot_product_rows(rec_t, to.tt_reconstruct(q)) for q in qs])
    assert int((bits(z["dot"]) != bits(dense)).sum()) == int(z["dense_differ"])
    assert int((bits(z["dot"]) != bits(so.similarity(so.DOT, ts, qs).T)).sum()) == int(z["swapped_differ"])
    assert np.abs(z["dot"].astype(np.float64) - dense).max() <= 1e-4 * np.abs(dense).max()
    with host_only():
        for name, op in (("dot", so.DOT), ("cosine", so.COSINE), ("euclidean", so.EUCLIDEAN)):
            assert same(tt.tt_similarity(op, lib_trains(qs), lib_trains(ts)), z[name]), name
        assert same(tt.tt_self_dot(lib_trains(ts)), z["self_t"]) and same(tt.tt_self_dot(lib_trains(qs)), z["self_q"])
