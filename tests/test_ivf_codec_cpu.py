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
