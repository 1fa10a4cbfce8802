"""tests/_tt_decompose_oracle.py against hand-derived values and the reference's own KATs, the library's host restatement of
tt_decompose against the twin bit for bit, the error texts, the new symbols, and the frozen fixture
tests/golden/tt_decompose_small.npz (docs/hnsw.md §21).  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import _tt_decompose_oracle as do

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "tt_decompose_small.npz")


def bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


class host_path:
    """NMN_HNSW_HOST_SEARCH=1: every call takes tt_decompose_host"""

    def __enter__(self):
        self.old = os.environ.get("NMN_HNSW_HOST_SEARCH")
        os.environ["NMN_HNSW_HOST_SEARCH"] = "1"

    def __exit__(self, *exc):
        if self.old is None:
            del os.environ["NMN_HNSW_HOST_SEARCH"]
        else:
            os.environ["NMN_HNSW_HOST_SEARCH"] = self.old


# ---- the twin against hand-derived values ----

def test_sums_fold_from_minus_zero_and_matmul_from_plus_zero():
    assert bits(do.dot(np.zeros(0, dtype=F), np.zeros(0, dtype=F))) == 0x80000000          # the empty sum is -0.0
    assert bits(do.dot([F(-0.0)], [F(1.0)])) == 0x80000000                                  # -0.0 + -0.0
    assert bits(do.dot([F(0.0)], [F(1.0)])) == 0                                            # -0.0 + +0.0
    assert bits(do.matmul(np.array([[-0.0]], dtype=F), np.array([[1.0]], dtype=F)))[0, 0] == 0   # +0.0 + -0.0
    # every add is rounded: (2^24 + 1) + 1 stays at 2^24 twice, 1 + 1 + 2^24 does not
    assert do.dot([F(4096.0), F(1.0), F(1.0)], [F(4096.0), F(1.0), F(1.0)]) == F(2 ** 24)
    assert do.dot([F(1.0), F(1.0), F(4096.0)], [F(1.0), F(1.0), F(4096.0)]) == F(2 ** 24 + 2)


def test_power_iteration_start_vector():
    """v_i = ((i * 7 + 3) % 13) / 13 - 0.5: 3, 10, 4, 11, 5, 12, 6, 0, 7, 1, 8, 2, 9, then again"""
    v = do.power_start(15)
    want = [3, 10, 4, 11, 5, 12, 6, 0, 7, 1, 8, 2, 9, 3, 10]
    assert np.array_equal(bits(v), bits(np.asarray([F(w) / F(13.0) - F(0.5) for w in want], dtype=F)))
    assert bits(v[7]) == bits(F(-0.5)) and v[1] > 0 > v[0]


def test_first_lcg_draws():
    """state = seed + 1, then state * 6364136223846793005 + 1442695040888963407 mod 2^64; a draw is (state >> 40) / 2^24"""
    g = do.Lcg(0)
    s1 = (1 * 6364136223846793005 + 1442695040888963407) % 2 ** 64
    s2 = (s1 * 6364136223846793005 + 1442695040888963407) % 2 ** 64
    assert s1 == 7806831264735756412
    d1, d2 = g.next_f32(), g.next_f32()
    assert float(d1) == (s1 >> 40) / 2 ** 24 and float(d2) == (s2 >> 40) / 2 ** 24
    assert 0.0 <= d1 < 1.0 and 0.0 <= d2 < 1.0
    m = do.gaussian_matrix(3, 3, 5)     # 9 values: 5 pairs, the last sine dropped
    assert m.shape == (3, 3) and np.isfinite(m).all()
    assert np.array_equal(bits(do.gaussian_matrix(3, 3, 5)), bits(m))
    assert not np.array_equal(bits(do.gaussian_matrix(3, 3, 6)), bits(m))


def test_two_by_two_rank_one_by_hand():
    """A = [3 4]^T [1 0] (rows [3 0], [4 0]) under shape (2, 2): v0 = normalize([3/13 - .5, 10/13 - .5]); u = A v = v_0 [3, 4],
    normalised to -[0.6, 0.8] (v_0 < 0) with sigma = 5 |v_0|; v = A^T u = [-5, 0] -> [-1, 0]; the second round gives u = [-3, -4]
    exactly, sigma = 5 exactly and u = -[0.6, 0.8]; the third confirms it and returns.  The residual after deflation is within
    rounding of zero, below 1e-4 * 5: rank 1, core 1 = -[0.6, 0.8], core 2 = 5 * [-1, 0]."""
    trace = []
    ranks, cores = do.tt_decompose(np.array([3, 0, 4, 0], dtype=F), (2, 2), 8, 1e-4, trace)
    assert ranks == [1, 1, 1] and trace[0] == 3
    assert np.array_equal(bits(cores[0].reshape(-1)), bits([F(-3.0) / F(5.0), F(-4.0) / F(5.0)]))
    assert cores[1].reshape(-1).tolist() == [-5.0, 0.0] and bits(cores[1].reshape(-1))[1] == 0x80000000   # 5 * -0.0


def test_zero_vectors_give_full_ranks_with_one_iteration_each():
    """sigma < abs_tol is 0 < 0: false, so nothing breaks; every power iteration returns at its first test"""
    trace = []
    ranks, cores = do.tt_decompose(np.zeros(24, dtype=F), (2, 3, 4), 8, 1e-4, trace)
    assert ranks == [1, 2, 4, 1] and trace == [1] * 6
    assert all(not c.any() for c in cores)
    assert do.tt_decompose(np.zeros(12, dtype=F), (3, 4), 8, 1e-4)[0] == [1, 3, 1]


def test_rank_one_tensor_breaks_after_one_value():
    rng = np.random.default_rng(5)
    for _ in range(4):
        assert do.tt_decompose(do.rank_one(rng, (2, 3, 4)), (2, 3, 4), 8, 1e-4)[0] == [1, 1, 1, 1]


def test_rank_zero_is_empty_matrix_with_a_step_to_come_and_ok_with_two_cores():
    rng = np.random.default_rng(6)
    failed = 0
    for _ in range(10):
        with pytest.raises(do.TTError) as e:
            do.tt_decompose(rng.standard_normal(64).astype(F), (4, 4, 4), 8, 0.9)
        failed += e.value.kind == "Decompose(EmptyMatrix)" and str(e.value) == "decomposition error: empty matrix"
        assert do.tt_decompose(do.rank_one(rng, (4, 4, 4)), (4, 4, 4), 8, 0.9)[0] == [1, 1, 1, 1]
    assert failed == 10
    ranks, cores = do.tt_decompose(rng.standard_normal(64).astype(F), (8, 8), 8, 0.9)
    assert ranks == [1, 0, 1] and [c.size for c in cores] == [0, 0]


def test_randomized_path_condition():
    assert do.takes_randomized_path(33, 34, 4) and not do.takes_randomized_path(32, 34, 4) and not do.takes_randomized_path(33, 32, 4)
    assert not do.takes_randomized_path(33, 34, 17) and do.takes_randomized_path(33, 34, 16)    # 2 rank < min(rows, cols)
    assert do.takes_randomized_path(64, 64, 8) and not do.takes_randomized_path(8, 512, 8) and not do.takes_randomized_path(64, 12, 8)


# ---- the twin against the reference's KATs ----

def test_kat_reconstruct_roundtrip():
    """test_tt_reconstruct_roundtrip (tensor_train.rs:743-769): sin(0.1 i), (4,4,4), rank 16, 1e-8, relative error < 0.1"""
    v = np.asarray([np.sin(F(i) * F(0.1)) for i in range(64)], dtype=F)
    ranks, cores = do.tt_decompose(v, (4, 4, 4), 16, 1e-8)
    rec = do.tt_reconstruct((4, 4, 4), ranks, cores)
    assert np.linalg.norm(rec - v) / np.linalg.norm(v) < 0.1


def test_kat_config_for_dim_optimal_shape_and_factorize_balanced():
    assert do.config_for_dim(4096)[0] == [8, 8, 8, 8] and do.config_for_dim(4096)[1] == 8
    assert do.optimal_shape(64) == [4, 4, 4] and do.optimal_shape(768) == [8, 8, 12] and do.optimal_shape(8192) == [8, 8, 8, 16]
    for n in (100, 1000, 97, 2, 3, 1, 360, 1 << 13 | 1, 30030):
        f = do.factorize_balanced(n)
        assert int(np.prod(f)) == n and f == sorted(f) and 1 <= len(f) <= 6
    assert do.factorize_balanced(0) == [] and do.factorize_balanced(1) == [1] and do.factorize_balanced(97) == [97]
    with pytest.raises(do.TTError, match="empty vector"):
        do.config_for_dim(0)


def test_kat_empty_and_shape_mismatch():
    with pytest.raises(do.TTError) as e:
        do.tt_decompose([], (4, 4), 8, 1e-4)
    assert e.value.kind == "EmptyVector" and str(e.value) == "empty vector"
    with pytest.raises(do.TTError) as e:
        do.tt_decompose(np.ones(64, dtype=F), (4, 4), 8, 1e-4)
    assert e.value.kind == "ShapeMismatch { dim: 64, shape: [4, 4], product: 16 }"
    assert str(e.value) == "dimension 64 cannot be reshaped to [4, 4] (product: 16)"
    with pytest.raises(do.TTError) as e:
        do.tt_decompose(np.ones(16, dtype=F), (4, 4), 0, 1e-4)
    assert e.value.kind == "InvalidRank"


def test_kat_qr_orthonormal():
    """test_qr_orthonormal (decompose.rs:764): Q^T Q is the identity within 1e-4; a dependent column is dropped"""
    y = do.gaussian_matrix(20, 5, 42)
    q = do.qr_orthonormalize(y)
    assert q.shape == (20, 5)
    assert np.abs(q.T.astype(np.float64) @ q.astype(np.float64) - np.eye(5)).max() < 1e-4
    y[:, 3] = 0.0
    assert do.qr_orthonormalize(y).shape == (20, 4)


# ---- the library's host path against the twin ----

def test_config_presets_equal_the_twin():
    from neumann_amd import TTConfig
    for dim in (1, 2, 3, 64, 97, 100, 128, 384, 768, 1000, 1122, 4096, 8192, 30030, 1 << 20):
        for name in do.PRESETS:
            c = getattr(TTConfig, name)(dim)
            shape, r, t = do.config_for_dim(dim, name)
            assert (c.shape, c.max_rank) == (shape, r) and bits(F(c.tolerance)) == bits(t), (dim, name)
            c.validate()
            assert c.max_storage == do.max_storage(shape, r)


CASES = do.gpu_cases()


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_host_restatement_equals_the_twin(case):
    from neumann_amd import TTConfig, tt
    _, shape, r, t, vectors = case
    with host_path():
        got = tt.tt_decompose_raw(vectors, TTConfig(shape, r, t))
    want = do.decompose_batch(vectors, shape, r, t)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2])
    assert np.array_equal(bits(got[3]), bits(want[3]))
    assert np.isfinite(got[3]).all()


def test_host_batch_rows_equal_one_vector_calls():
    from neumann_amd import TTConfig, tt
    shape, r, t, v = do.big_batch()
    cfg = TTConfig(shape, r, t)
    with host_path():
        status, ranks, off, cores = tt.tt_decompose_raw(v, cfg)
        assert len({tuple(x) for x in ranks.tolist()}) >= 3
        for q in (0, 1, 2, 51, 299):
            s1, r1, o1, c1 = tt.tt_decompose_raw(v[q], cfg)
            assert s1[0] == status[q] and np.array_equal(r1[0], ranks[q])
            assert np.array_equal(bits(c1), bits(cores[int(off[q]):int(off[q + 1])]))
        tts = tt.tt_decompose(v[:4], cfg)
        assert [x.ranks for x in tts] == ranks[:4].tolist()
        rec = tt.tt_reconstruct([tts[0]])[0]
    assert np.linalg.norm(rec.astype(np.float64) - v[0]) / np.linalg.norm(v[0]) < 1e-3     # rank-one: within rounding


def test_error_texts_and_statuses():
    from neumann_amd import NeumannGpuError, TTConfig, _capi, tt
    with host_path():
        with pytest.raises(NeumannGpuError, match="empty vector"):
            tt.tt_decompose(np.zeros((2, 0), dtype=F), TTConfig([4, 4]))
        with pytest.raises(NeumannGpuError, match=re.escape("dimension 64 cannot be reshaped to [4, 4] (product: 16)")):
            tt.tt_decompose(np.ones(64, dtype=F), TTConfig([4, 4]))
        with pytest.raises(NeumannGpuError, match=re.escape("invalid TT-rank: must be >= 1")):
            tt.tt_decompose(np.ones(16, dtype=F), TTConfig([4, 4], max_rank=0))
        with pytest.raises(NeumannGpuError, match="empty vector"):
            TTConfig.for_dim(0)
        # the tolerance is validate()'s, not tt_decompose's
        with pytest.raises(NeumannGpuError, match="invalid tolerance"):
            TTConfig([4, 4], 8, 1.5).validate()
        assert tt.tt_decompose(np.arange(16, dtype=F), TTConfig([4, 4], 8, 1.5))[0].ranks == [1, 0, 1]
        rng = np.random.default_rng(9)
        v = np.vstack([rng.standard_normal((1, 64)).astype(F), do.rank_one(rng, (4, 4, 4))[None]])
        cfg = TTConfig([4, 4, 4], 8, 0.9)
        with pytest.raises(tt.TTDecomposeError, match="vector 0: decomposition error: empty matrix"):
            tt.tt_decompose(v, cfg)
        out = tt.tt_decompose(v, cfg, return_status=True)
        assert isinstance(out[0], tt.TTDecomposeError) and out[0].kind == "Decompose(EmptyMatrix)" and out[1].ranks == [1, 1, 1, 1]
        # a capacity the trains do not fit in writes nothing
        lib = _capi.load()
        p = lambda a: C.c_void_p(a.ctypes.data)   # noqa: E731
        sh, st, rk, off, cores = np.array([4, 4, 4], np.uint32), np.full(2, 7, np.uint32), np.zeros((2, 4), np.uint32), \
            np.zeros(3, np.uint64), np.full(8, 7, F)
        code = lib.nmn_tt_decompose(p(v), 2, 64, p(sh), 3, 8, C.c_float(0.9), p(st), p(rk), p(off), p(cores), 8)
        assert code == _capi.ERR_INVALID_ARGUMENT and "cores_cap" in lib.nmn_last_error().decode() and (st == 7).all() and (cores == 7).all()
    lim = tt.decompose_limits()
    assert lim[0] == 8 and lim[3] * 4 <= 64 * 1024
    assert tt.decompose_lds_floats(TTConfig([8, 8, 12])) <= lim[3] and tt.decompose_lds_floats(TTConfig([8, 8, 8, 8])) <= lim[3]
    assert tt.decompose_lds_floats(TTConfig([256, 256], 64)) is None


def test_new_symbols_are_exported_declared_and_bound():
    from neumann_amd import GpuHnsw, _capi, tt
    lib = _capi.load()
    header = open(os.path.join(ROOT, "include", "neumann_gpu.h")).read()
    ffi = open(os.path.join(ROOT, "integration", "rust", "ffi.rs")).read()
    for name in ("nmn_tt_config_for_dim", "nmn_tt_max_storage", "nmn_tt_decompose", "nmn_tt_decompose_device", "nmn_tt_decompose_limits",
                 "nmn_tt_decompose_lds_floats", "nmn_hnsw_search_tt_dense", "nmn_hnsw_insert_tt_dense", "nmn_hnsw_insert_batch_tt"):
        assert hasattr(lib, name), name
        assert re.search(rf"\b{name}\s*\(", header), name
        assert name in _capi.SIGNATURES, name
        assert re.search(rf"pub fn {name}\(", ffi), name
    for m in ("search_tt_dense", "insert_tt_dense", "insert_batch_tt"):
        assert callable(getattr(GpuHnsw, m))
    for m in ("TTConfig", "tt_decompose", "decompose_limits"):
        assert hasattr(tt, m)


def test_golden_fixture_is_the_twin():
    z = np.load(GOLDEN)
    assert os.path.getsize(GOLDEN) < 100 * 1024
    for name, shape, r, t, vectors in CASES:
        if vectors.shape[1] > 128:
            continue
        status, ranks, off, cores = do.decompose_batch(vectors, shape, r, t)
        assert np.array_equal(bits(z[name + "_vectors"]), bits(vectors)), name
        assert np.array_equal(z[name + "_status"], status) and np.array_equal(z[name + "_ranks"], ranks), name
        assert np.array_equal(z[name + "_core_off"], off) and np.array_equal(bits(z[name + "_cores"]), bits(cores)), name
    assert np.array_equal(bits(z["gaussian_34x9_seed_1057"]), bits(do.gaussian_matrix(34, 9, 33 * 31 + 34)))
