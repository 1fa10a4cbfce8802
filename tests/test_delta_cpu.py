"""Delta vectors without a GPU (docs/delta.md): the twin tests/_delta_oracle.py against values derived by hand and against the known
answers of the reference's own unit tests, the library's host restatement (min_device_rows = never) against the twin on every case
of tests/_delta_cases.py, every refusal, the frozen fixture tests/golden/delta_small.npz, and the plumbing of the new symbols."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from tests import _delta_cases as dc
from tests import _delta_oracle as do

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "delta_small.npz")
HOST = dc.NEVER
SYMBOLS = ("nmn_delta_options_default", "nmn_delta_limits", "nmn_archetypes_create", "nmn_archetypes_destroy", "nmn_archetypes_set_options",
           "nmn_archetypes_register", "nmn_archetypes_discover", "nmn_archetypes_len", "nmn_archetypes_dim", "nmn_archetypes_max",
           "nmn_archetypes_get", "nmn_archetypes_magnitude_sq", "nmn_archetypes_find_best", "nmn_archetypes_analyze_coverage",
           "nmn_archetypes_encode_batch", "nmn_delta_set_from_parts", "nmn_delta_set_destroy", "nmn_delta_set_len", "nmn_delta_set_nnz",
           "nmn_delta_set_arrays", "nmn_delta_set_compression_ratio", "nmn_delta_set_memory_bytes", "nmn_delta_set_decode",
           "nmn_delta_set_magnitudes", "nmn_delta_set_dot_dense", "nmn_delta_set_cosine_dense", "nmn_delta_set_dot_same_archetype",
           "nmn_archetypes_to_device", "nmn_delta_set_to_device", "nmn_archetypes_find_best_device", "nmn_delta_set_dot_dense_device",
           "nmn_delta_set_cosine_dense_device")


# ---- the twin itself ------------------------------------------------------------------------------------------------------------

def test_sums_fold_from_minus_zero_and_accumulators_from_plus_zero():
    empty = do.DeltaVector(0, 4, [], [])
    zero_arch, neg_q = np.zeros(4, dtype=F), -np.ones(4, dtype=F)
    assert dc.bits(do.sum_sq_rows(np.zeros((1, 0), dtype=F)))[0] == 0x80000000             # an empty `.sum()` is -0.0
    assert dc.bits(empty.dot_dense(neg_q, zero_arch)) == 0x80000000                        # -0.0 + -0.0
    assert dc.bits(empty.dot_dense(-neg_q, zero_arch)) == 0                                # the products are +0.0: -0.0 + 0.0
    assert dc.bits(empty.sparse_delta_dot(empty)) == 0                                     # `let mut result = 0.0`
    assert dc.bits(empty.dot_same_archetype(empty, zero_arch, F(-0.0))) == 0               # ... which makes the four-term sum +0.0
    # one sequential chain: 2^24 + 1 is 2^24, then - 2^24: 0; the other order gives 1
    big = F(2.0 ** 24)
    a = do.DeltaVector(0, 3, [0, 1, 2], [big, 1.0, -big])
    b = do.DeltaVector(0, 3, [0, 2, 1], [big, -big, 1.0])
    ones = np.ones(3, dtype=F)
    assert a.dot_dense_with_precomputed(ones, F(0.0)) == 0.0 and b.dot_dense_with_precomputed(ones, F(0.0)) == 1.0


def test_size_of_delta_vector_and_the_reference_bounds():
    """72 = 8 + 8 + 24 + 24 + 8 (docs/delta.md §1).  The reference's own tests bound it: test_memory_bytes (two entries of 100
    dimensions: memory_bytes() < 100, so the size is below 88) and test_compression_ratio (one entry of 100 dimensions: ratio > 5.0,
    so 400 / (size + 6) > 5: the size is below 74); test_compression_ratio_no_deltas only asks for a positive ratio."""
    two = do.DeltaVector.from_dense_with_reference([1.0, 1.0] + [0.0] * 98, [0.0] * 100, 0, 0.001)
    assert two.nnz() == 2 and two.memory_bytes() == 84 < 100
    v = np.ones(100, dtype=F)
    v[0] = 0.9
    one = do.DeltaVector.from_dense_with_reference(v, np.ones(100), 0, 0.001)
    assert one.nnz() == 1 and one.memory_bytes() == 78 and one.compression_ratio() > 5.0
    assert dc.same(one.compression_ratio(), F(F(400.0) / F(78.0)))
    assert do.DeltaVector(0, 0, [], []).compression_ratio() == 1.0
    from neumann_amd import delta
    assert delta.DELTA_VECTOR_BYTES == do.SIZE_OF_DELTA_VECTOR == 72 and delta.MAX_DIMENSION == do.MAX_DIMENSION
    lib, _ = dc.registries(100, np.ones((1, 100)), mdr=HOST)
    s = lib.encode_batch(v[None, :], 0.001)
    assert s.memory_bytes().tolist() == [78] and dc.same(s.compression_ratio(), [one.compression_ratio()])


def test_known_answers_of_the_reference_unit_tests():
    z = np.load(GOLDEN)
    # test_delta_vector_from_dense_with_reference / _reconstruct / _dot_product (delta_vector.rs, mod tests)
    archetype, dense = z["kat_archetype"], z["kat_dense"]
    d = do.DeltaVector.from_dense_with_reference(dense, archetype, 0, 0.001)
    assert d.positions.tolist() == z["kat_positions"].tolist() and dc.same(d.deltas, z["kat_deltas"])
    assert dc.same(d.to_dense(archetype), z["kat_reconstructed"])
    assert np.abs(d.to_dense(archetype) - dense).max() < 0.001                            # the reference's own assertion
    assert dc.same(d.dot_dense(z["kat_query"], archetype), z["kat_dot"])
    from neumann_amd import DeltaSet
    lib, _ = dc.registries(4, archetype[None, :], mdr=HOST)
    s = lib.encode_batch(dense[None, :], 0.001)
    assert s.positions.tolist() == z["kat_positions"].tolist() and dc.same(s.deltas, z["kat_deltas"])
    assert dc.same(s.to_dense()[0], z["kat_reconstructed"]) and dc.same(s.dot_dense(z["kat_query"])[0, 0], z["kat_dot"])
    assert isinstance(s, DeltaSet)
    # test_find_best_archetype: the axes as archetypes, a vector near each
    lib3, twin3 = dc.registries(3, np.eye(3), mdr=HOST)
    for v, want in (([0.9, 0.1, 0.0], 0), ([0.1, 0.9, 0.1], 1), ([0.0, 0.2, 0.95], 2)):
        assert lib3.find_best_archetype(v)[0] == want == twin3.find_best_archetype(v)[0]
    assert dc.same(lib3.find_best_archetype([0.9, 0.1, 0.0])[1], twin3.find_best_archetype([0.9, 0.1, 0.0])[1])
    assert lib3.find_best_archetype([0.9, 0.1, 0.0])[1] > 0.9


# ---- the host restatement against the twin ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dim", dc.FIND_DIMS)
@pytest.mark.parametrize("K", dc.FIND_KS)
def test_host_find_best(dim, K):
    dc.check_find_best(HOST, dim, K, 130)


@pytest.mark.parametrize("N", dc.FIND_NS)
def test_host_find_best_rows(N):
    dc.check_find_best(HOST, 65, 9, N)


def test_host_find_best_specials_and_empty_registry():
    dc.check_find_best_specials(HOST)
    dc.check_empty_registry(HOST)


@pytest.mark.parametrize("threshold", dc.THRESHOLDS)
@pytest.mark.parametrize("dim", dc.ENCODE_DIMS)
def test_host_encode(dim, threshold):
    dc.check_encode(HOST, dim, threshold, dim % 2 == 1)
    if dim == 65:
        dc.check_encode(HOST, dim, threshold, False)


def test_host_encode_at_the_largest_dimension():
    dc.check_encode_wide(HOST)


def test_host_coverage():
    dc.check_coverage(HOST)


@pytest.mark.parametrize("nq", (1, 2, 5))
def test_host_scores(nq):
    dc.check_score(HOST, nq)


def test_host_scores_of_encoded_sets_and_wide_queries():
    from neumann_amd import delta
    dc.check_score_encoded(HOST)
    lds = delta.limits()[1]
    dc.check_score_lds_limit(HOST, lds)
    dc.check_score_lds_limit(HOST, lds + 1)


def test_host_from_parts_sets_and_pairs():
    dc.check_parts(HOST)


def test_refusals_and_their_texts():
    dc.check_refusals(HOST)
    dc.check_refusals(dc.ALWAYS)          # refused before any path is chosen: no device is touched


def test_default_sends_everything_to_the_host_or_to_a_measured_crossover():
    """docs/delta.md §7: the default of min_device_rows is the crossover the measurements show; this test runs where there is no
    GPU, so a registry with the default options must answer small calls on the host"""
    from neumann_amd import ArchetypeRegistry, delta
    assert delta.default_options() >= 1024
    reg = ArchetypeRegistry(4, 2)
    reg.register([1, 0, 0, 0])
    assert reg.find_best_archetype([2, 0, 0, 0]) == (0, F(1.0))


# ---- the fixture ------------------------------------------------------------------------------------------------------------------

def test_golden_fixture_is_the_twin_and_tells_the_naive_sums_apart():
    from tests.golden import make_golden_delta as mk
    z = np.load(GOLDEN)
    want = mk.compute()
    assert sorted(z.files) == sorted(want)
    for k in z.files:
        assert z[k].dtype == want[k].dtype and z[k].shape == want[k].shape, k
        assert dc.same(z[k], want[k]) if z[k].dtype == F else np.array_equal(z[k], want[k]), k
    assert int(z["pairwise_differ"]) > 0 and int(z["plus_zero_differ"]) > 0
    lib, twin = dc.registries(z["archetypes"].shape[1], z["archetypes"], mdr=HOST)
    ids, sims = lib.find_best_batch(z["rows"])
    assert np.array_equal(ids, z["best_ids"]) and dc.same(sims, z["best_sims"])
    s = lib.encode_batch(z["rows"], float(z["threshold"]), True)
    a = s.arrays()
    assert np.array_equal(a["indptr"], z["indptr"]) and np.array_equal(a["positions"], z["positions"]) and dc.same(a["deltas"], z["deltas"])
    assert dc.same(a["cached_magnitudes"], z["cached"])
    assert dc.same(s.dot_dense(z["queries"]), z["dot"]) and dc.same(s.cosine_similarity_dense(z["queries"]), z["cosine"])
    assert dc.same(s.to_dense(), z["decoded"])
    u = lib.encode_batch(z["rows"], float(z["threshold"]), False)
    assert dc.same(u.magnitudes(), z["magnitudes_uncached"])
    got, ok = lib.dot_deltas_same_archetype(s, s, z["pairs"])
    assert np.array_equal(ok, z["pair_ok"]) and dc.same(got[ok], z["pair_dot"][z["pair_ok"]])


# ---- plumbing -----------------------------------------------------------------------------------------------------------------------

def test_new_symbols_are_exported_declared_and_bound():
    import neumann_amd
    from neumann_amd import _capi, build, delta
    lib = _capi.load()
    header = open(os.path.join(ROOT, "include", "neumann_gpu.h")).read()
    ffi = open(os.path.join(ROOT, "integration", "rust", "ffi.rs")).read()
    for name in SYMBOLS:
        assert hasattr(lib, name), name
        assert re.search(rf"\b{name}\s*\(", header), name
        assert name in _capi.SIGNATURES, name
        assert re.search(rf"pub fn {name}\(", ffi), name
    declared = set(re.findall(r"\b(nmn_(?:delta|archetypes)_\w+)\s*\(", header))
    assert declared == set(SYMBOLS), declared ^ set(SYMBOLS)
    assert build.SOURCES["nmn_delta.hip"] == ["-ffp-contract=off", "-fhip-fp32-correctly-rounded-divide-sqrt"]
    for cls in ("ArchetypeRegistry", "DeltaSet", "DeltaVectorError", "CoverageStats"):
        assert getattr(neumann_amd, cls) is getattr(delta, cls), cls
    for fn in ("register", "discover_archetypes", "find_best_archetype", "encode", "encode_batch", "decode", "dot_delta_dense",
               "dot_deltas_same_archetype", "analyze_coverage", "__len__", "get", "magnitude_sq", "find_best_device"):
        assert callable(getattr(delta.ArchetypeRegistry, fn)), fn
    for fn in ("from_parts", "to_dense", "magnitudes", "dot_dense", "cosine_similarity_dense", "compression_ratio", "memory_bytes",
               "dot_dense_device", "cosine_similarity_dense_device", "arrays"):
        assert callable(getattr(delta.DeltaSet, fn)), fn
    assert delta.limits() == (65535, 8192, 8, 256)
    gpu_index = open(os.path.join(ROOT, "integration", "rust", "gpu_index.rs")).read()
    for item in ("pub struct GpuArchetypeRegistry", "pub struct GpuDeltaSet", "pub fn find_best", "pub fn encode_batch", "pub fn dot_dense"):
        assert item in gpu_index, item
    n_funcs = len(re.findall(r"^\s+pub fn nmn_\w+\(", ffi, flags=re.M))
    assert f"{n_funcs} functions in all" in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def test_generated_ffi_is_current():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_rust_ffi.py"), "--check"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_the_new_sources_read_no_environment_variable():
    for rel in ("neumann_amd/csrc/nmn_delta.hip", "neumann_amd/delta.py", "tools/delta_bench.py"):
        text = open(os.path.join(ROOT, rel)).read()
        assert "getenv" not in text and "environ" not in text, rel
        assert not re.search(r"\"NMN_[A-Z0-9_]+\"", text), rel
