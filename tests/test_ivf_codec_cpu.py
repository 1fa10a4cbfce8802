"""IVF-PQ / IVF-Binary without a GPU: the numpy restatement (tests/_ivf_codec_oracle.py) against the reference's own unit
tests (tensor_store/src/pq.rs:432-667, binary_quantization.rs:238-440, ivf.rs:748-790), the new C-ABI symbols, and
estimate_ivf_memory (vector_engine/src/lib.rs:2821-2851), which is host arithmetic."""
import re

import numpy as np
import pytest

from tests import _ivf_codec_oracle as co

F = np.float32
FAST = co.KMeansConfig(max_iterations=2, convergence_threshold=1.0, seed=42, init_method="random")  # ivf.rs:589-596


def create_test_vectors(n, dim):  # pq.rs:432-440
    return np.array([[F(((i * 7 + j * 13) % 100) / 100.0) for j in range(dim)] for i in range(n)], dtype=F)


def test_pq_config_presets():  # pq.rs pq_config_default / high_compression / high_recall
    assert (co.PQConfig().num_subspaces, co.PQConfig().num_centroids) == (8, 256)
    assert co.PQConfig.high_compression().num_subspaces == 4
    assert co.PQConfig.high_recall().num_subspaces == 32
    from neumann_amd.engine import IVFBuildOptions, PQConfig
    assert (PQConfig.default().num_subspaces, PQConfig.default().num_centroids) == (8, 256)
    assert PQConfig.high_compression().num_subspaces == 4 and PQConfig.high_recall().num_subspaces == 32
    assert IVFBuildOptions.pq(16).storage[0] == "pq" and IVFBuildOptions.binary(16).storage == ("binary", "sign")
    assert IVFBuildOptions.flat(16).storage == ("flat",) and IVFBuildOptions().storage == ("flat",)
    with pytest.raises(ValueError):
        IVFBuildOptions.binary(16, "mode")


def test_pq_codebook_train_and_roundtrip():  # pq_codebook_train_basic, pq_encode_decode_roundtrip, pq_dimension_validation
    V = create_test_vectors(100, 64)
    cb = co.PQCodebook.train(V, co.PQConfig(8, 16, FAST))
    assert (cb.num_subspaces, cb.subspace_dim, cb.original_dim, cb.num_centroids) == (8, 8, 64, 16)
    enc = cb.encode(V[0])
    dec = cb.decode(enc)
    assert len(enc) == 8 and len(dec) == 64
    assert np.sqrt(((V[0] - dec) ** 2).sum()) < 5.0
    assert co.PQCodebook.train(create_test_vectors(10, 64), co.PQConfig(8, 256, FAST)).num_centroids == 10  # K' = min(K, n)


def test_pq_adc_matches_decoded_distance():  # pq_adc_table_correctness
    V = create_test_vectors(50, 32)
    cb = co.PQCodebook.train(V, co.PQConfig(4, 8, FAST))
    table = cb.compute_adc_table(V[0])
    enc = cb.encode(V[1])
    true = np.sqrt(co.sq_dist_rows(cb.decode(enc)[None, :], V[0])[0])
    assert abs(co.adc_distance(table, enc) - true) < 0.01
    assert co.adc_distances(table, enc[None, :])[0] == co.adc_distance(table, enc)


def test_pq_edge_cases():  # pq_empty_vectors, pq_dimension_not_divisible, pq_adc_empty_query
    cb = co.PQCodebook.train(np.zeros((0, 64), F), co.PQConfig())
    assert cb.original_dim == 0 and cb.subspace_dim == 0
    with pytest.raises(ValueError, match="must be divisible"):
        co.PQCodebook.train(create_test_vectors(10, 65), co.PQConfig(8, 256, FAST))
    assert co.adc_squared_distance(cb.compute_adc_table([]), np.zeros(8, np.uint8)) == co.F32_MAX
    # K' = 0: every distance is sqrt(f32::MAX) (pq.rs:392-413)
    cb0 = co.PQCodebook.train(create_test_vectors(10, 16), co.PQConfig(4, 0, FAST))
    assert cb0.num_centroids == 0 and list(cb0.encode(create_test_vectors(1, 16)[0])) == [0] * 4
    assert co.adc_distance(cb0.compute_adc_table(create_test_vectors(1, 16)[0]), np.zeros(4, np.uint8)) == np.sqrt(co.F32_MAX)


def test_pq_code_wraps_above_256():  # `k as u8`
    cb = co.PQCodebook(1, 1, 300, np.arange(300, dtype=F).reshape(1, 300, 1), 1)
    assert cb.encode(np.array([299.0], F))[0] == 299 - 256


def test_binary_from_dense():  # binary_from_dense_sign / _mean / _median, binary_large_dimension
    assert co.from_dense([0.1, -0.5, 0.3, -0.2, 0.8, -0.1, 0.0, 0.4], "sign")[0] == 0b1001_0101
    assert co.from_dense([1.0, 2.0, 3.0, 4.0], "mean")[0] == 0b1100
    assert co.from_dense([1.0, 5.0, 2.0, 4.0, 3.0], "median")[0] == 0b0_1010
    big = co.from_dense([1.0 if i % 2 == 0 else -1.0 for i in range(1536)], "sign")
    assert len(big) == 24 and sum(bin(int(w)).count("1") for w in big) == 768


def test_binary_threshold_and_distance():  # binary_threshold_compute / _empty, binary_hamming_*, binary_normalized_distance
    v = [1.0, 2.0, 3.0, 4.0, 5.0]
    assert co.threshold(v, "sign") == 0.0 and co.threshold(v, "mean") == 3.0 and co.threshold(v, "median") == 3.0
    assert all(co.threshold([], m) == 0.0 for m in ("sign", "mean", "median"))
    assert co.threshold([1.0, 2.0, 3.0, 4.0], "median") == 2.5  # midpoint of the two middle elements
    assert co.hamming([0b1010_1010], [0b0101_0101]) == 8 and co.hamming([0b1111], [0b1111]) == 0
    assert co.normalized_distance([0b1111_0000], [0b0000_1111], 8) == 1.0
    # Mean folds sequentially in f32: differs from a pairwise / f64 sum on these values
    x = np.array([1e8, 1.0, -1e8, 1.0], F)
    assert co.threshold(x, "mean") == F(F(F(F(1e8) + F(1.0)) + F(-1e8)) + F(1.0)) / F(4)


@pytest.mark.parametrize("storage", ["pq", "binary"])
def test_ivf_integration(storage):  # ivf_pq_integration / ivf_binary_integration (ivf.rs:748-790)
    V = create_test_vectors(20, 32)
    idx = co.IVFCoded(4, storage, pq_config=co.PQConfig(4, 8, FAST), nprobe=2, kmeans=FAST)
    idx.train(V)
    for v in V:
        idx.add(v)
    ids, d = idx.search(V[0], 5)
    assert ids and len(ids) <= 5 and np.all(np.diff(d) >= 0)
    assert sum(idx.cluster_sizes()) == 20


def test_new_symbols_exported():
    from neumann_amd import _capi
    lib = _capi.load()
    for n in ("nmn_ivf_storage_default", "nmn_ivf_build_ex", "nmn_ivf_create_ex", "nmn_ivf_storage_kind", "nmn_ivf_pq_codewords",
              "nmn_ivf_pq_codebook", "nmn_ivf_codes", "nmn_ivf_hbm_bytes", "nmn_engine_build_ivf_index_ex",
              "nmn_engine_estimate_ivf_memory"):
        assert hasattr(lib, n), n
    import ctypes as C
    s = _capi.IvfStorage()
    lib.nmn_ivf_storage_default(C.byref(s))
    assert (s.kind, s.pq_num_subspaces, s.pq_num_centroids, s.binary_threshold) == (_capi.IVF_FLAT, 8, 256, _capi.BINARY_SIGN)
    assert (s.pq_kmeans.max_iterations, s.pq_kmeans.seed, s.pq_kmeans.init_method) == (100, 42, 1)
    assert s.pq_kmeans.convergence_threshold == F(1e-4)
    # the header declares the same struct layout as the binding
    import os
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "neumann_gpu.h")).read()
    body = re.search(r"typedef struct nmn_ivf_storage \{(.*?)\} nmn_ivf_storage;", hdr, flags=re.S).group(1)
    fields = re.findall(r"\b(\w+);", body)
    assert fields == [f[0] for f in _capi.IvfStorage._fields_]


def test_estimate_ivf_memory_matches_reference_formula():  # lib.rs:2821-2851
    from neumann_amd.engine import IVFBuildOptions, PQConfig, VectorEngine
    e = VectorEngine()
    for opt in (IVFBuildOptions.flat(10), IVFBuildOptions.pq(10), IVFBuildOptions.binary(10)):
        assert e.estimate_ivf_memory(opt) == 0  # empty engine
    for i in range(37):
        e.store_embedding(f"k{i}", [float(i + j) for j in range(100)])
    n, d = 37, 100
    assert e.estimate_ivf_memory(IVFBuildOptions.flat(10)) == co.estimate_ivf_memory(n, d, 10, "flat") == 10 * d * 4 + n * d * 4 + n * 8
    assert e.estimate_ivf_memory(IVFBuildOptions.pq(10, PQConfig.high_recall())) == co.estimate_ivf_memory(n, d, 10, "pq", 32)
    assert e.estimate_ivf_memory(IVFBuildOptions.pq(7)) == 7 * d * 4 + n * 8 + n * 8
    assert e.estimate_ivf_memory(IVFBuildOptions.binary(10, "median")) == co.estimate_ivf_memory(n, d, 10, "binary") == \
        10 * d * 4 + n * 2 * 8 + n * 8


# ---- the batch helpers (assign_rows, encode_rows, from_dense_rows, normalized_distances, add_rows) against their scalar
# originals: the GPU tests of the long paths (tests/test_gpu_ivf_codec_paths.py) rest on them ---------------------------
BQ_METHODS = ["sign", "mean", "median"]


def _rows(n, d, seed):
    return np.random.default_rng(seed).standard_normal((n, d)).astype(F)


def _codebook(M, K, sub, seed):
    return co.PQCodebook(sub, M, K, _rows(M * K, sub, seed).reshape(M, K, sub), M * sub)


def _encode_each(cb, R):
    return np.stack([cb.encode(r) for r in R])


@pytest.mark.parametrize("M,K,dim", [(4, 16, 16), (16, 16, 16), (1, 300, 8), (8, 256, 96), (2, 16, 8)])
def test_encode_rows_random(M, K, dim):
    cb = _codebook(M, K, dim // M, seed=20)
    R = _rows(40, dim, seed=21)
    got = cb.encode_rows(R)
    assert got.dtype == np.uint8 and np.array_equal(got, _encode_each(cb, R))


def test_encode_rows_first_of_tied_codewords_wins():
    cb = _codebook(2, 12, 3, seed=22)
    cb.centroids[:, 7] = cb.centroids[:, 2]   # codewords 2, 7 and 9 are one point: 2 must win
    cb.centroids[:, 9] = cb.centroids[:, 2]
    cb.centroids[0, 0] = cb.centroids[0, 11]  # ... and 0 before 11
    R = _rows(30, 6, seed=23)
    R[:10] = np.concatenate([cb.centroids[0, 2], cb.centroids[1, 9]])  # rows that sit on the tied codewords
    R[10:14] = np.concatenate([cb.centroids[0, 11], cb.centroids[1, 7]])
    got = cb.encode_rows(R)
    assert np.array_equal(got, _encode_each(cb, R))
    assert got[0].tolist() == [2, 2] and got[10].tolist() == [0, 2] and not np.isin(got, (7, 9, 11)).any()


def test_encode_rows_wraps_above_256_codewords():
    cb = co.PQCodebook(1, 1, 300, np.arange(300, dtype=F).reshape(1, 300, 1), 1)
    R = np.array([[299.0], [256.0], [255.0], [0.2], [1000.0]], F)
    got = cb.encode_rows(R)
    assert got[:, 0].tolist() == [43, 0, 255, 0, 43] and np.array_equal(got, _encode_each(cb, R))
    cb = _codebook(2, 300, 2, seed=24)
    R = _rows(60, 4, seed=25)
    assert np.array_equal(cb.encode_rows(R), _encode_each(cb, R))


def test_encode_rows_every_distance_at_or_above_f32_max_gives_code_0():
    """`dist < best_dist` from f32::MAX never fires when a subspace's every distance is f32::MAX or +inf: code 0, although
    the first minimum (np.argmin) sits elsewhere.  Subspace 0: codeword 1 is at distance f32::MAX exactly,
    (2^64 (1 - 2^-24))^2 + (2^52)^2 = 2^128 (1 - 2^-23) + 2^104 = f32::MAX with both squares and the sum exact; the others
    overflow.  Subspace 1 is ordinary."""
    cb = _codebook(2, 4, 2, seed=26)
    cb.centroids[0] = [[3e38, 0.0], [0.0, 0.0], [3e38, 0.0], [-3e38, 0.0]]
    R = _rows(5, 4, seed=27)
    R[:, 0], R[:, 1] = np.nextafter(F(2.0 ** 64), F(0.0)), F(2.0 ** 52)
    R[3, 0] = F(2.0 ** 64)  # this row overflows against every codeword
    with np.errstate(over="ignore"):
        d = np.stack([co.sq_dist_rows(cb.centroids[0], r[:2]) for r in R])
        assert d[0, 1] == co.F32_MAX and np.isposinf(d[0, [0, 2, 3]]).all() and np.isposinf(d[3]).all()
        assert int(np.argmin(d[0])) == 1  # what a bare argmin would have stored
        got = cb.encode_rows(R)
        assert np.array_equal(got, _encode_each(cb, R))
    assert not got[:, 0].any() and got[:, 1].any()
    R[4, 1] = F(2.0 ** 51)  # one row just below f32::MAX: codeword 1 wins for it alone
    with np.errstate(over="ignore"):
        got = cb.encode_rows(R)
        assert np.array_equal(got, _encode_each(cb, R))
    assert got[:, 0].tolist() == [0, 0, 0, 0, 1]


def test_assign_rows():
    cents = _rows(7, 12, seed=28)
    cents[5] = cents[1]  # a duplicated centroid: the first wins
    V = _rows(200, 12, seed=29)
    V[:20] = cents[1] + F(0.001)
    got = co.assign_rows(V, cents)
    assert got.tolist() == [co.nearest_centroid(v, cents) for v in V] and 5 not in got.tolist() and 1 in got.tolist()


def _bq_rows(dim, seed):
    """random rows plus the edges of the threshold: ties at the middle ranks, a one-ulp gap there, zeros of both signs"""
    V = _rows(24, dim, seed)
    mid = dim // 2
    V[1] = F(0.75)                                              # all equal
    V[2] = np.where(np.arange(dim) % 2 == 0, F(0.0), F(-0.0))    # zeros of both signs
    V[3] = -np.abs(V[3]) - F(0.5)                                # all negative
    s = np.sort(V[4])
    if dim >= 2:
        s[mid - 1] = s[mid]                                      # both middle ranks equal ...
        V[4] = s[np.random.default_rng(seed + 1).permutation(dim)]
        s = np.sort(V[5])
        s[mid - 1] = np.nextafter(s[mid], F(-np.inf), dtype=F)   # ... and one ulp apart
        V[5] = s[np.random.default_rng(seed + 2).permutation(dim)]
        V[6, ::2], V[6, 1::2] = F(0.0), F(-0.0)                  # zeros around the middle of a mixed row
        V[6, : dim // 4] = F(-1.0)
        V[6, dim - dim // 4:] = F(1.0)
    if dim >= 3:
        V[7] = np.repeat(V[7, : (dim + 2) // 3], 3)[:dim]        # every value three times
    return V


@pytest.mark.parametrize("method", BQ_METHODS)
@pytest.mark.parametrize("dim", [1, 2, 7, 8, 63, 64, 65, 130])
def test_from_dense_rows(method, dim):
    V = _bq_rows(dim, seed=30 + dim)
    got = co.from_dense_rows(V, method)
    assert got.dtype == np.uint64 and got.shape == (len(V), (dim + 63) // 64)
    assert np.array_equal(got, np.stack([co.from_dense(v, method) for v in V]))
    thr = co.thresholds_rows(V, method)
    want = np.array([co.threshold(v, method) for v in V], F)
    assert np.array_equal(thr, want)  # (values: -0.0 == +0.0, which `v > t` cannot tell apart either)


def test_from_dense_rows_mean_is_sequential():
    x = np.array([[1e8, 1.0, -1e8, 1.0], [1.0, 1.0, 1e8, -1e8]], F)
    assert co.thresholds_rows(x, "mean").tolist() == [0.25, 0.0]
    assert np.array_equal(co.from_dense_rows(x, "mean"), np.stack([co.from_dense(v, "mean") for v in x]))


def test_normalized_distances():
    for dim in (1, 8, 64, 65, 130, 1000):
        W = co.from_dense_rows(_rows(50, dim, seed=40 + dim), "sign")
        W[3] = W[0]
        W[4] = ~W[0] & co.from_dense_rows(np.ones((1, dim), F), "sign")[0]  # every bit differs
        got = co.normalized_distances(W[0], W, dim)
        want = np.array([co.normalized_distance(W[0], w, dim) for w in W], F)
        assert got.dtype == F and np.array_equal(got.view(np.uint32), want.view(np.uint32))
        assert got[3] == 0.0 and got[4] == 1.0
    assert co.normalized_distances(np.zeros(0, np.uint64), np.zeros((3, 0), np.uint64), 0).tolist() == [0.0] * 3


def _same_state(a, b):
    assert a.assign == b.assign and a.lists == b.lists and len(a.codes) == len(b.codes)
    assert all(type(x) is int for x in a.assign) and all(type(i) is int for lst in a.lists for i in lst)
    for x, y in zip(a.codes, b.codes):
        assert x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x, y)


@pytest.mark.parametrize("storage,arg", [("pq", (4, 16)), ("pq", (2, 300)), ("binary", "sign"), ("binary", "mean"),
                                         ("binary", "median")])
def test_add_rows_equals_repeated_add(storage, arg):
    dim = 8
    cents = _rows(3, dim, seed=50) * F(4.0)
    V = (_rows(150, dim, seed=51) + cents[np.random.default_rng(52).integers(0, 3, 150)]).astype(F)
    V[40:60] = V[39]  # duplicates
    V[70] = np.where(np.arange(dim) % 2 == 0, F(0.0), F(-0.0))
    pair = []
    for _ in range(2):
        if storage == "pq":
            o = co.IVFCoded(3, "pq", pq_config=co.PQConfig(*arg), nprobe=2)
            o.set_trained(cents, _codebook(arg[0], arg[1], dim // arg[0], seed=53))
        else:
            o = co.IVFCoded(3, "binary", threshold=arg, nprobe=2)
            o.set_trained(cents)
        pair.append(o)
    one, many = pair
    for v in V:
        one.add(v)
    got = many.add_rows(V[:100])
    assert got.tolist() == one.assign[:100]
    many.add_rows(V[100:])  # a second batch continues the ids
    _same_state(many, one)
    for q in (V[39], V[3] + F(0.5)):
        (i1, d1), (i2, d2) = one.search(q, 200, 3), many.search(q, 200, 3)
        assert i1 == i2 and np.array_equal(d1.view(np.uint32), d2.view(np.uint32))
    if storage == "binary":  # the search's vectorised distances against the scalar function, in candidate order
        ids, d = one.search(V[3], 200, 3)
        qb = co.from_dense(V[3], arg)
        assert [float(x) for x in d] == [float(co.normalized_distance(qb, one.codes[i], dim)) for i in ids]


def _source(name):
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    return open(os.path.join(root, "neumann_amd", "csrc", name)).read()


def test_codec_path_thresholds_match_the_kernels():
    """tests/test_gpu_ivf_codec_paths.py places each case on a kernel path by these thresholds: a retuned kernel must say so
    here, not let a case slide back onto a path the older tests already cover"""
    from tests import test_gpu_ivf_codec_paths as paths
    codec, ivf = _source("nmn_ivf_codec.hip"), _source("nmn_ivf.hip")

    def one(pattern, text):
        found = re.findall(pattern, text)
        assert len(found) >= 1 and len(set(found)) == 1, (pattern, found)
        return found[0]

    assert int(one(r"constexpr uint32_t kCodecRowsPerBlock = (\d+);", codec)) == paths.SCAN_ROWS_PER_BLOCK
    a, b = one(r"constexpr size_t kLdsBudget = (\d+) \* (\d+);", codec)
    assert int(a) * int(b) == paths.LDS_BUDGET
    # both launchers take the LDS variant at `lds <= kLdsBudget` (inclusive: a table of exactly the budget stays in LDS)
    assert len(re.findall(r"if \(lds <= kLdsBudget\) hipLaunchKernelGGL\(pq_(?:encode|scan)_kernel<true>", codec)) == 2
    assert "const size_t lds = (size_t)K * subdim * 4;" in codec and "const size_t lds = (size_t)M * Kt * 4;" in codec
    assert "Kt = std::min<uint32_t>(K, 256)" in codec
    # launch_bq_quantize: `r0 += 65535` rows per launch and the same count in the min()
    assert {int(x) for x in re.findall(r"for \(uint64_t r0 = 0; r0 < n; r0 \+= (\d+)\)", codec)} == {paths.BQ_ROWS_PER_LAUNCH}
    assert int(one(r"std::min<uint64_t>\((\d+), n - r0\)", codec)) == paths.BQ_ROWS_PER_LAUNCH
    # launch_pq_residual: at most 8192 blocks of 256 threads; launch_pq_encode: at most 1024 blocks of 256 rows
    blocks = one(r"std::min<uint64_t>\(\(n \* dim \+ 255\) / 256, (\d+)\)", codec)
    assert int(blocks) == paths.RESIDUAL_MAX_BLOCKS and paths.RESIDUAL_BLOCK == 256
    assert "hipLaunchKernelGGL(pq_residual_kernel, dim3(blocks), dim3(256)" in codec
    assert int(one(r"std::min<uint64_t>\(\(n \+ 255\) / 256, (\d+)\), M\)", codec)) * 256 == paths.ENCODE_ROWS_PER_GRID
    # codec_add: rows per stage
    assert int(one(r"const uint64_t kStage = std::min<uint64_t>\(n, (\d+)\);", ivf)) == paths.ADD_STAGE_ROWS
    # the 16-byte code reads
    assert "(M & 15u) == 0" in codec and paths.CODE_VECTOR_BYTES == 16
