"""tests/_hnsw_bin_oracle.py held by hand: the arithmetic of EmbeddingStorage::Binary nodes (docs/hnsw.md §18), the three
thresholds, the surface of the new entries, and the frozen golden file.  No GPU."""
import os
import re
from fractions import Fraction

import numpy as np
import pytest

from tests import _hnsw_bin_oracle as hb
from tests import _hnsw_oracle as ho
from tests import _ivf_codec_oracle as co

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "hnsw_bin_small.npz")


def bits(x):
    return int(np.asarray(x, dtype=F).reshape(()).view(np.uint32))


def index_of(rows, metric, threshold="sign"):
    return hb.build(np.asarray(rows, dtype=F), ho.HNSWConfig.high_speed().with_distance_metric(metric), threshold)


# ---- dim 3, Hamming 1: the two sides of Cosine -----------------------------------------------------------------------------------
def test_cosine_pruning_side_bits_dim3_hamming1():
    """1 - (1 - 1/3).  1/3 rounds up to 11184811 * 2^-25 (0x3EAAAAAB); 1 - that = 22369621 * 2^-25 is a tie between two f32 of
    [0.5, 1) and goes to the even 11184810 * 2^-24 (0x3F2AAAAA); 1 - that = 5592406 * 2^-24, exact: 0x3EAAAAAC."""
    a, b = co.from_dense([1, 1, 1], "sign"), co.from_dense([1, 1, -1], "sign")
    assert co.hamming(a, b) == 1
    assert bits(hb.similarity(a, b, 3)) == 0x3F2AAAAA
    assert bits(hb.pruning_cosine(a, b, 3)) == 0x3EAAAAAC
    idx = index_of([[1, 1, 1], [1, 1, -1]], ho.COSINE)
    assert bits(idx._dist_pairs(0, [1])[0]) == 0x3EAAAAAC


def test_cosine_query_side_bits_dim3_hamming1():
    """1 - 1 / (sqrt3 * sqrt3).  The dot of the two +-1 rows is 1 + 1 - 1 = 1; sqrt(3f32) = 0x3FDDB3D7 = 1.7320507764816284, below
    the real root; its square 2.99999989... rounds to 3.0 (half an ulp of [2, 4) is 1.19e-7); 1 / 3 = 0x3EAAAAAB; 1 - that is the
    tie of the test above: 0x3F2AAAAA."""
    idx = index_of([[1, 1, 1], [1, 1, -1]], ho.COSINE)
    q = idx.get_vector(1)
    assert q.tolist() == [1.0, 1.0, -1.0]
    qmag = idx._qmag(q)
    assert bits(qmag) == 0x3FDDB3D7 == bits(hb.mag_self(3))
    assert bits(F(qmag) * hb.mag_self(3)) == 0x40400000
    assert bits(idx._dist_query([0], q, qmag)[0]) == 0x3F2AAAAA


def test_the_two_sides_differ():
    """about h/d against about 2h/d: one formula on both sides would break or create ties and build another graph"""
    idx = index_of([[1, 1, 1], [1, 1, -1]], ho.COSINE)
    q = idx.get_vector(1)
    assert bits(idx._dist_query([0], q, idx._qmag(q))[0]) != bits(idx._dist_pairs(1, [0])[0])
    rng = np.random.default_rng(5)
    rows = rng.standard_normal((40, 20)).astype(F)
    idx = index_of(rows, ho.COSINE)
    q = idx.get_vector(0)
    a = idx._dist_query(list(range(1, 40)), q, idx._qmag(q))
    b = idx._dist_pairs(0, list(range(1, 40)))
    assert np.allclose(a, 2 * b, atol=1e-5) and np.count_nonzero(a != b) == np.count_nonzero(b)
    for metric in (ho.EUCLIDEAN, ho.DOT_PRODUCT):            # ... where these two metrics use one arithmetic on both sides
        idx = index_of(rows, metric)
        q = idx.get_vector(0)
        assert idx._dist_query(list(range(1, 40)), q, F(0)).tobytes() == idx._dist_pairs(0, list(range(1, 40))).tobytes()


# ---- Euclidean and DotProduct of two +-1 rows ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [1, 5, 8, 13, 64, 65, 200])
def test_euclidean_of_two_pm1_rows_is_sqrt_4h(dim):
    """every term is 0 or (+-2)^2 = 4, every partial sum an integer below 2^24: the sum is 4h exactly, then one correctly rounded
    sqrt"""
    rng = np.random.default_rng(dim)
    rows = rng.standard_normal((12, dim)).astype(F)
    idx = index_of(rows, ho.EUCLIDEAN)
    ids = list(range(12))
    for a in range(12):
        h = np.array([co.hamming(idx.words[a], idx.words[b]) for b in ids])
        want = np.sqrt((4 * h).astype(F))
        assert idx._dist_query(ids, idx.get_vector(a), F(0)).tobytes() == want.tobytes()
        assert idx._dist_pairs(a, ids).tobytes() == want.tobytes()
    idx = index_of(rows, ho.DOT_PRODUCT)                     # and the dot is dim - 2h, negated
    for a in range(12):
        h = np.array([co.hamming(idx.words[a], idx.words[b]) for b in ids])
        assert idx._dist_pairs(a, ids).tobytes() == (-((dim - 2 * h).astype(F))).tobytes()     # (a dot of +0.0 is -0.0 negated)


# ---- mag_self ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim,want", [(2, 0x3FB504F3), (3, 0x3FDDB3D7), (771, 0x41DE2296)])
def test_mag_self_is_the_correctly_rounded_root_of_the_dimension(dim, want):
    m = hb.mag_self(dim)
    assert bits(m) == want
    lo, hi = Fraction(float(np.nextafter(m, F(0)))), Fraction(float(np.nextafter(m, F(np.inf))))
    x = Fraction(float(m))
    assert ((x + lo) / 2) ** 2 < dim < ((x + hi) / 2) ** 2   # dim lies between the squares of the two rounding boundaries
    idx = index_of(np.ones((2, dim)), ho.COSINE)             # ... and it is what Cosine divides by, whatever the row's bits
    q = np.full(dim, 0.5, dtype=F)
    qmag = idx._qmag(q)
    dot = ho.dot_product_rows(idx.rows[:1], q)[0]
    assert bits(idx._dist_query([0], q, qmag)[0]) == bits(F(1.0) - dot / (m * qmag))


def test_a_zero_query_gives_one():
    idx = index_of(np.random.default_rng(1).standard_normal((9, 13)), ho.COSINE)
    q = np.zeros(13, dtype=F)
    assert idx._qmag(q) == 0
    assert idx._dist_query(list(range(9)), q, idx._qmag(q)).tolist() == [1.0] * 9
    res = idx.search_with_ef(q, 4, 50)
    assert len(res) == 4 and all(s == F(0.0) for _, s in res)                      # to_similarity: 1 - 1


# ---- the scalar tail stays out of the chains --------------------------------------------------------------------------------------
def test_dim13_tail_follows_the_lane_sum():
    """q = [1e8, -1e8, 0 x 6 | 1, 0 x 4] on the all-ones row.  The chains hold 1e8 and -1e8, their sum is 0, the tail adds 1: dot 1.
    Had element 8 entered chain 0, 1e8 + 1 would have rounded to 1e8 (an ulp there is 8) and the dot would be 0."""
    idx = index_of(np.ones((1, 13)), ho.DOT_PRODUCT)
    assert idx.words[0].tolist() == [0x1FFF]
    q = np.zeros(13, dtype=F)
    q[0], q[1], q[8] = 1e8, -1e8, 1.0
    assert idx._dist_query([0], q, F(0)).tolist() == [-1.0]
    assert F(F(1e8) + F(1.0)) == F(1e8)
    # the same for a clear tail bit: the row's element 8 is -1, the term is -q[8]
    idx = index_of(np.concatenate([np.ones(8), [-1.0], np.ones(4)])[None, :], ho.DOT_PRODUCT)
    assert idx.words[0].tolist() == [0x1EFF]
    assert idx._dist_query([0], q, F(0)).tolist() == [1.0]
    # Euclidean: (1 - 1e8)^2 and (1 + 1e8)^2 in two chains, six 1s, then the tail's (-1 - 1)^2 = 4 and four 1s after the lane sum
    idx = index_of(np.concatenate([np.ones(8), [-1.0], np.ones(4)])[None, :], ho.EUCLIDEAN)
    d0, d1 = F(F(1.0) - F(1e8)), F(F(1.0) + F(1e8))
    r = F(-0.0)
    for t in (d0 * d0, d1 * d1) + (F(1.0),) * 6 + (F(4.0),) + (F(1.0),) * 4:
        r = F(r + t)
    assert bits(idx._dist_query([0], q, F(0))[0]) == bits(np.sqrt(r))


# ---- the three thresholds (binary_quantization.rs:41-65, its own tests 237-266) -------------------------------------------------------
def test_thresholds():
    assert co.from_dense([0.1, -0.5, 0.3, -0.2, 0.8, -0.1, 0.0, 0.4], "sign").tolist() == [0b10010101]   # 237-246
    assert co.from_dense([1.0, 2.0, 3.0, 4.0], "mean").tolist() == [0b1100]                              # 248-256: mean 2.5
    assert co.from_dense([1.0, 5.0, 2.0, 4.0, 3.0], "median").tolist() == [0b01010]                      # 258-266: median 3
    assert co.from_dense([1, 5, 2, 4, 3], "sign").tolist() == [0b11111]
    assert co.from_dense([1, 5, 2, 4, 3], "mean").tolist() == [0b01010]                                  # mean 3: 3 > 3 is false
    assert co.from_dense([1, 2, 3, 4], "sign").tolist() == [0b1111]
    assert co.from_dense([1, 2, 3, 4], "median").tolist() == [0b1100]                                    # midpoint(2, 3) = 2.5
    assert co.threshold([1, 2, 3, 4], "median") == F(2.5)
    for method in ("sign", "mean", "median"):                # a row of zeros of either sign: nothing is above the threshold
        assert co.from_dense([0.0, -0.0, 0.0, -0.0, -0.0], method).tolist() == [0]
        assert co.from_dense([-0.0, 0.0, -0.0, 0.0], method).tolist() == [0]
    # the midpoint goes through f64: (a + b) / 2 of two huge elements does not overflow
    big = np.array([3e38, 3e38, -1.0, 1.0], dtype=F)
    assert co.threshold(big, "median") == F((float(F(1.0)) + float(F(3e38))) / 2)
    assert co.from_dense(big, "median").tolist() == [0b0011]
    # padding bits of the last word are zero; to_dense gives +-1
    w = co.from_dense(np.ones(70), "sign")
    assert w.tolist() == [(1 << 64) - 1, 0x3F]
    assert hb.to_dense(co.from_dense([3, -3, 0, 2], "sign"), 4).tolist() == [1.0, -1.0, -1.0, 1.0]


def test_memory_bytes_and_get_vector():
    rows = np.random.default_rng(2).standard_normal((7, 130)).astype(F)
    idx = index_of(rows, ho.COSINE, "mean")
    assert idx.memory_bytes() == 7 * 3 * 8
    assert np.array_equal(idx.words[:7], co.from_dense_rows(rows, "mean"))
    for i in range(7):
        assert idx.get_vector(i).tobytes() == idx.rows[i].tobytes()
        assert set(idx.get_vector(i).tolist()) <= {1.0, -1.0}


# ---- the surface -------------------------------------------------------------------------------------------------------------------
NEW_SYMBOLS = ["nmn_hnsw_create_binary", "nmn_hnsw_binary_threshold", "nmn_hnsw_binary_row"]


def test_new_symbols_are_exported_declared_and_bound():
    from neumann_amd import _capi
    lib = _capi.load()
    gpu_h = open(os.path.join(ROOT, "include", "neumann_gpu.h")).read()
    ffi = open(os.path.join(ROOT, "integration", "rust", "ffi.rs")).read()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
        assert re.search(rf"\b{name}\s*\(", gpu_h), name
        assert re.search(rf"pub fn {name}\(", ffi), name
        assert name in _capi.SIGNATURES
    assert re.search(r"#define NMN_HNSW_STORAGE_BINARY 3\b", gpu_h) and _capi.HNSW_STORAGE_BINARY == 3
    assert re.search(r"pub const NMN_HNSW_STORAGE_BINARY: i32 = 3;", ffi)
    assert "pub fn new_binary(" in open(os.path.join(ROOT, "integration", "rust", "gpu_index.rs")).read()


# ---- the frozen golden file ------------------------------------------------------------------------------------------------------------
def test_golden_corpus_and_words():
    z = np.load(GOLDEN)
    rows, queries = ho.golden_corpus()
    assert z["rows"].tobytes() == rows.tobytes() and z["queries"].tobytes() == queries.tobytes()
    assert z["rows"].shape == (800, 20) and z["queries"].shape == (64, 20)
    assert int(z["k"]) == hb.GOLDEN_K == 10 and int(z["ef"]) == hb.GOLDEN_EF == 50
    for t in hb.GOLDEN_THRESHOLDS:
        assert np.array_equal(z[f"words_{t}"], co.from_dense_rows(rows, t))
        assert np.array_equal(z[f"words_{t}"][37], co.from_dense(rows[37], t))


@pytest.mark.parametrize("metric", hb.GOLDEN_METRICS)
@pytest.mark.parametrize("threshold", hb.GOLDEN_THRESHOLDS)
def test_golden_file_matches_the_oracle(threshold, metric):
    z = np.load(GOLDEN)
    want = hb.golden_case(z["rows"], z["queries"], threshold, metric)
    assert want, "no arrays"
    for name, arr in want.items():
        got = z[name]
        assert got.dtype == np.asarray(arr).dtype and got.shape == np.asarray(arr).shape, name
        assert got.tobytes() == np.asarray(arr).tobytes(), name
