"""tests/_hnsw_q8_oracle.py held to hand-derived cases and to exact rational arithmetic, and the quantized HNSW surface (symbols,
header, Rust FFI, HNSWBuildOptions presets) — no GPU needed."""
import os
import re
from fractions import Fraction

import numpy as np

from tests import _hnsw_oracle as ho
from tests import _hnsw_q8_oracle as q8

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def bits(x):
    return np.ascontiguousarray(x, dtype=F).view(np.uint32).tolist()


# ---- from_dense / dequantize (hnsw.rs:324-368) ----------------------------------------------------------------------------------
def test_from_dense_rounds_halves_away_from_zero():
    codes, scale, mn = q8.from_dense([0.0, 0.5, 1.5, 2.5, 255.0])
    assert scale == F(1.0) and mn == F(0.0)                       # (255 - 0) / 255
    assert codes.tolist() == [0, 1, 2, 3, 255]                    # half to even would give 0, 2, 2
    # the largest f32 below 0.5 rounds to 0; floor(x + 0.5) in f32 would give 1
    below_half = np.nextafter(F(0.5), F(0.0))
    assert F(below_half + F(0.5)) == F(1.0)
    assert q8.round_half_away([below_half, 0.5, 1.4999999, -0.5, -2.5, 254.5]).tolist() == [0.0, 1.0, 1.0, -1.0, -3.0, 255.0]
    codes, scale, mn = q8.from_dense([0.0, below_half, 255.0])
    assert codes.tolist() == [0, 0, 255]


def test_from_dense_constant_and_tiny_range():
    codes, scale, mn = q8.from_dense([1.5] * 11)
    assert scale == F(1.0) and mn == F(1.5) and codes.tolist() == [0] * 11
    assert bits(q8.dequantize(codes, scale, mn)) == bits([1.5] * 11)
    # a range below f32::EPSILON (2^-24 < 2^-23): scale 1.0, every code 0, every element dequantized to the minimum
    v = np.asarray([0.5, 0.5 + 2.0 ** -24, 0.5], dtype=F)
    assert v[1] != v[0]
    codes, scale, mn = q8.from_dense(v)
    assert scale == F(1.0) and mn == F(0.5) and codes.tolist() == [0, 0, 0]
    # a range of exactly EPSILON is NOT below it
    v = np.asarray([1.0, 1.0 + 2.0 ** -23], dtype=F)
    codes, scale, mn = q8.from_dense(v)
    assert scale == F(F(2.0 ** -23) / F(255.0)) and codes.tolist() == [0, 255]
    # zeros: scale 1.0, magnitude 0
    codes, scale, mn = q8.from_dense(np.zeros(9, F))
    assert scale == F(1.0) and mn == F(0.0) and not codes.any()


# ---- the fused multiply-add --------------------------------------------------------------------------------------------------------
def fraction_to_f32(x):
    """round a Fraction to the nearest f32, ties to even (normal and subnormal range)"""
    if x == 0:
        return F(0.0)
    sign = -1 if x < 0 else 1
    x = abs(x)
    e = x.numerator.bit_length() - x.denominator.bit_length()
    if Fraction(2) ** e > x:
        e -= 1
    assert Fraction(2) ** e <= x < Fraction(2) ** (e + 1)
    quantum = Fraction(2) ** (max(e, -126) - 23)
    n = x / quantum
    lo = n.numerator // n.denominator
    rem = n - lo
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and lo % 2 == 1):
        lo += 1
    return F(sign * float(lo * quantum))          # exact: at most 24 significant bits


def test_fma_rounds_once():
    rng = np.random.default_rng(0xF3A)
    n = 3000
    a = (rng.standard_normal(n) * 10.0 ** rng.integers(-6, 7, n)).astype(F)
    b = (rng.standard_normal(n) * 10.0 ** rng.integers(-6, 7, n)).astype(F)
    c = (rng.standard_normal(n) * 10.0 ** rng.integers(-6, 7, n)).astype(F)
    # cancelling triples: c is -(a * b) rounded to f32, or a neighbour of it — the sum is the product's rounding error
    k = n // 2
    p = (a[:k].astype(np.float64) * b[:k].astype(np.float64))
    c[:k] = (-p).astype(F)
    c[:k:3] = np.nextafter(c[:k:3], F(np.inf))
    c[1:k:3] = np.nextafter(c[1:k:3], F(-np.inf))
    # double-rounding triples: a * b = 1 + 2^-11 + 2^-24 sits exactly halfway between two f32; a c far below the f64 grid decides
    # the side, and an f64 sum loses it
    for j, tiny in enumerate((2.0 ** -60, -2.0 ** -60, 2.0 ** -70, -2.0 ** -80)):
        a[k + j], b[k + j], c[k + j] = F(1 + 2.0 ** -12) * F(2.0 ** j), F(1 + 2.0 ** -12), F(tiny * 2.0 ** j)
    got = q8.fma32(a, b, c)
    differs_from_unfused = 0
    differs_from_double = 0
    for i in range(n):
        exact = Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i]))
        want = fraction_to_f32(exact)
        assert got[i].tobytes() == want.tobytes(), (i, a[i], b[i], c[i], got[i], want)
        differs_from_unfused += F(a[i] * b[i]) + c[i] != want
        differs_from_double += F(np.float64(a[i]) * np.float64(b[i]) + np.float64(c[i])) != want
    assert differs_from_unfused > 100      # the cases tell a fused from an unfused evaluation ...
    assert differs_from_double >= 2        # ... and from f64-then-f32 (double rounding)
    # scalars and broadcasting
    assert q8.fma32(F(3.0), F(4.0), F(5.0)) == F(17.0)
    assert q8.fma32(np.asarray([1, 2], F), F(2.0), F(1.0)).tolist() == [3.0, 5.0]


# ---- dot_dense / squared_magnitude / euclidean_distance_dense by hand --------------------------------------------------------------
V = np.asarray([0, 51, 102, 153, 204, 255, 0, 255, 51, 102], dtype=F)   # one chunk of eight and a tail of two
Y = np.arange(1, 11, dtype=F)


def test_quantized_formulas_on_integer_vectors():
    # codes == V (scale 1, min 0): sum(V * Y) = 7089, sum(Y) = 55, sum(V^2) = 221085, sum(V) = 1173, sum(Y^2) = 385
    codes, scale, mn = q8.from_dense(V)
    assert codes.tolist() == V.tolist() and scale == F(1.0) and mn == F(0.0)
    assert q8.dot_dense(codes, scale, mn, Y)[0] == F(7089.0)
    assert q8.squared_magnitude(codes, scale, mn)[0] == F(221085.0)
    # ||x - y||^2 = 221085 + 385 - 2 * 7089 = 207292
    assert bits(q8.euclidean_distance_dense(codes, scale, mn, Y)) == bits(np.sqrt(F(207292.0)))
    assert float(np.sum((V.astype(np.float64) - Y) ** 2)) == 207292.0
    # min 3: dot gains 3 * 55, the squared magnitude 2 * 1 * 3 * 1173 + 9 * 10
    codes, scale, mn = q8.from_dense(V + F(3.0))
    assert codes.tolist() == V.tolist() and scale == F(1.0) and mn == F(3.0)
    assert q8.dot_dense(codes, scale, mn, Y)[0] == F(7089.0 + 165.0)
    assert q8.squared_magnitude(codes, scale, mn)[0] == F(221085.0 + 7038.0 + 90.0)
    assert bits(q8.dequantize(codes, scale, mn)) == bits(V + F(3.0))
    # scale 2 (range 510): the codes are V again
    codes, scale, mn = q8.from_dense(V * F(2.0))
    assert codes.tolist() == V.tolist() and scale == F(2.0) and mn == F(0.0)
    assert q8.dot_dense(codes, scale, mn, Y)[0] == F(2 * 7089.0)
    assert q8.squared_magnitude(codes, scale, mn)[0] == F(4 * 221085.0)
    # a negative fused sum is clamped to 0 before the square root
    assert q8.euclidean_distance_dense(codes, scale, mn, Y, x_sq=F(0.0))[0] == F(0.0)


def test_index_distances_and_bookkeeping():
    for metric in (ho.COSINE, ho.EUCLIDEAN, ho.DOT_PRODUCT):
        idx = q8.HNSWQ8Index(ho.HNSWConfig(distance_metric=metric))
        idx.insert(V)
        idx.insert(np.zeros(10, F))
        assert idx.memory_bytes() == 2 * (16 + 10)
        assert bits(idx.get_vector(0)) == bits(V) and bits(idx.rows[0]) == bits(V)
        d = idx._dist_query([0, 1], Y, idx._qmag(Y))
        if metric == ho.DOT_PRODUCT:
            assert d.tolist() == [-7089.0, 0.0]
        elif metric == ho.EUCLIDEAN:
            assert bits(d) == bits([np.sqrt(F(207292.0)), np.sqrt(F(385.0))])
        else:   # magnitude_immutable = simd::magnitude(dequantize()); a zero row is at distance 1.0
            want = F(1.0) - F(7089.0) / (np.sqrt(F(221085.0)) * np.sqrt(F(385.0)))
            assert bits(d) == bits([want, 1.0])
            assert idx._dist_query([0], np.zeros(10, F), idx._qmag(np.zeros(10, F)))[0] == F(1.0)
        assert idx.distance_evals >= 2


def test_the_two_sides_differ_in_bits():
    """query side (quantized formulas) against pruning side (dense arithmetic on dequantized rows): a build that used one formula
    for both would build another graph"""
    rng = np.random.default_rng(3)
    rows = rng.standard_normal((60, 20)).astype(F)
    for metric in (ho.COSINE, ho.EUCLIDEAN, ho.DOT_PRODUCT):
        idx = q8.build(rows, ho.HNSWConfig.high_speed().with_distance_metric(metric))
        ids = list(range(1, 60))
        q = idx.rows[0].copy()
        a = idx._dist_query(ids, q, idx._qmag(q))
        b = idx._dist_pairs(0, ids)
        assert np.count_nonzero(a.view(np.uint32) != b.view(np.uint32)) > 5
        assert np.allclose(a, b, rtol=1e-3, atol=1e-3)


# ---- the surface -------------------------------------------------------------------------------------------------------------------
NEW_GPU_SYMBOLS = ["nmn_hnsw_create_with_storage", "nmn_hnsw_storage", "nmn_hnsw_quantized_row", "nmn_hnsw_get_vector",
                   "nmn_hnsw_memory_stats"]
NEW_ENGINE_SYMBOLS = ["nmn_engine_build_hnsw_index_with_options", "nmn_hnsw_build_options_default",
                      "nmn_hnsw_build_options_memory_optimized", "nmn_hnsw_build_options_high_recall",
                      "nmn_hnsw_build_options_sparse_optimized"]


def test_new_symbols_are_exported_declared_and_bound():
    from neumann_amd import _capi
    lib = _capi.load()
    gpu_h = open(os.path.join(ROOT, "include", "neumann_gpu.h")).read()
    eng_h = open(os.path.join(ROOT, "include", "neumann_engine.h")).read()
    ffi = open(os.path.join(ROOT, "integration", "rust", "ffi.rs")).read()
    for name in NEW_GPU_SYMBOLS:
        assert hasattr(lib, name), name
        assert re.search(rf"\b{name}\s*\(", gpu_h), name
        assert re.search(rf"pub fn {name}\(", ffi), name
        assert name in _capi.SIGNATURES
    for name in NEW_ENGINE_SYMBOLS:
        assert hasattr(lib, name), name
        assert re.search(rf"\b{name}\s*\(", eng_h), name
    assert "pub struct nmn_hnsw_memstats" in ffi


def test_build_options_presets():
    """HNSWBuildOptions, vector_engine/src/lib.rs:860-932 — the Python class and the C presets"""
    import ctypes as C

    from neumann_amd import HNSWBuildOptions, HNSWConfig, _capi
    lib = _capi.load()
    want = {"default": ("dense", HNSWConfig.default()), "memory_optimized": ("quantized", HNSWConfig.high_speed()),
            "high_recall": ("dense", HNSWConfig.high_recall()), "sparse_optimized": ("auto", HNSWConfig.default())}
    code = {"dense": _capi.HNSW_STORAGE_DENSE, "auto": _capi.HNSW_STORAGE_AUTO, "quantized": _capi.HNSW_STORAGE_QUANTIZED}
    for preset, (storage, cfg) in want.items():
        o = getattr(HNSWBuildOptions, preset)()
        assert o.storage == storage
        co = _capi.HnswBuildOptions()
        getattr(lib, f"nmn_hnsw_build_options_{preset}")(C.byref(co))
        assert co.storage == code[storage] and co.reserved == 0
        for c in (o.hnsw_config, co.hnsw_config):
            assert (c.m, c.m0, c.ef_construction, c.ef_search, c.max_nodes) == (cfg.m, cfg.m0, cfg.ef_construction, cfg.ef_search,
                                                                                 cfg.max_nodes)
            assert abs(c.ml - cfg.ml) < 1e-15 and c.sparsity_threshold == 0.5 and int(c.distance_metric) == 0
    assert (want["memory_optimized"][1].m, want["memory_optimized"][1].ef_construction, want["memory_optimized"][1].ef_search) == (8, 100, 20)
    o = HNSWBuildOptions.new().with_storage("auto").with_sparsity_threshold(0.7)                      # lib.rs:2413-2415
    assert o.storage == "auto" and o.hnsw_config.sparsity_threshold == 0.7
    o = HNSWBuildOptions().with_hnsw_config(HNSWConfig.high_recall()).with_storage("quantized")
    assert o.storage == "quantized" and o.hnsw_config.m == 32
