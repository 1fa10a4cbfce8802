"""The top-k search over a delta set without a GPU (docs/delta.md §8): the twin tests/_deltaset_oracle.py against answers derived by
hand, the library's host path (min_device_rows = never) against the twin on every case of tests/_deltaset_cases.py, and the plumbing
of the new symbols."""
import os
import re

import numpy as np
import pytest

from tests import _delta_cases as dc
from tests import _deltaset_cases as sc
from tests import _deltaset_oracle as dso

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = dc.NEVER
SYMBOLS = ("nmn_deltaset_limits", "nmn_deltaset_search", "nmn_deltaset_search_scratch_bytes", "nmn_deltaset_search_device",
           "nmn_deltaset_encode_device", "nmn_deltaset_host_arrays_present")


# ---- the twin itself ------------------------------------------------------------------------------------------------------------

def test_key_map_and_order_by_hand():
    inf = np.inf
    v = np.asarray([1.0, -0.0, np.nan, -inf, 0.0, inf, -1.0, 1.0, -np.nan], dtype=F)
    keys = dso.score_to_key(v)
    assert keys.tolist() == [0xBF800000, 0x80000000, 1, 0x007FFFFF, 0x80000000, 0xFF800000, 0x407FFFFF, 0xBF800000, 1]
    rows, scores, count = dso.top_k(v, 11)
    assert rows.tolist() == [5, 0, 7, 1, 4, 6, 3, 2, 8, -1, -1] and count == 9
    assert dc.bits(scores)[:9].tolist() == dc.bits(v)[[5, 0, 7, 1, 4, 6, 3, 2, 8]].tolist()          # each row's own bits
    assert np.isneginf(scores[9:]).all()
    assert dso.top_k(v, 2)[0].tolist() == [5, 0] and dso.top_k(v[:0], 2)[0].tolist() == [-1, -1]
    # the keys order as the scores do, on a sweep of patterns of every kind
    rng = np.random.default_rng(0)
    w = rng.integers(0, 2 ** 32, size=4000, dtype=np.uint64).astype(np.uint32).view(F)
    w = w[~np.isnan(w)]
    k = dso.score_to_key(w).astype(np.int64)
    i, j = rng.integers(0, w.size, size=(2, 20000))
    assert ((w[i] < w[j]) == (k[i] < k[j])).all() and ((w[i] == w[j]) == (k[i] == k[j])).all()
    assert k.min() > dso.KEY_NAN


# ---- the host path against the twin ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", sc.SIZES)
def test_host_search_sizes(n):
    sc.check_sizes(HOST, n)


@pytest.mark.parametrize("k", (4096, 4097))
def test_host_search_at_the_select_limit(k):
    sc.check_k_border(HOST, k)


def test_host_search_ties():
    sc.check_all_equal(HOST)
    sc.check_tie_runs(HOST)
    sc.check_zeros(HOST)


def test_host_search_special_scores():
    sc.check_specials(HOST)


@pytest.mark.parametrize("which", ("low", "mid", "top"))
def test_host_search_radix_patterns(which):
    sc.check_radix(HOST, which)


@pytest.mark.parametrize("nq", (1, 2, 5))
def test_host_search_of_scored_sets(nq):
    sc.check_scored_set(HOST, nq)


def test_host_search_of_encoded_and_unsorted_sets():
    sc.check_encoded_and_unsorted(HOST)


def test_host_search_empty_set_and_refusals():
    sc.check_empty_set_and_refusals(HOST)
    sc.check_empty_set_and_refusals(dc.ALWAYS)          # refused, or answered without a row, before any path is chosen


def test_host_search_in_blocks_of_queries():
    sc.check_query_blocks(HOST)


def test_host_search_around_the_single_query_threshold():
    sc.check_single_query_threshold(HOST)


def test_host_search_two_threads_and_history():
    sc.check_two_threads(HOST)
    sc.check_history(HOST)


# ---- plumbing -----------------------------------------------------------------------------------------------------------------------

def test_search_symbols_are_exported_declared_and_bound():
    from neumann_amd import _capi, delta
    lib = _capi.load()
    header = open(os.path.join(ROOT, "include", "neumann_gpu.h")).read()
    ffi = open(os.path.join(ROOT, "integration", "rust", "ffi.rs")).read()
    for name in SYMBOLS:
        assert hasattr(lib, name), name
        assert re.search(rf"\b{name}\s*\(", header), name
        assert name in _capi.SIGNATURES, name
        assert re.search(rf"pub fn {name}\(", ffi), name
    assert set(re.findall(r"\b(nmn_deltaset_\w+)\s*\(", header)) == set(SYMBOLS)
    for fn in ("search", "search_device", "search_scratch_bytes"):
        assert callable(getattr(delta.DeltaSet, fn)), fn
    assert callable(delta.ArchetypeRegistry.encode_batch_device) and isinstance(delta.DeltaSet.host_arrays_present, property)
    assert delta.search_limits() == (4096, 4096, 256 << 20, 1 << 18)
    gpu_index = open(os.path.join(ROOT, "integration", "rust", "gpu_index.rs")).read()
    assert "pub fn search(" in gpu_index[gpu_index.index("impl GpuDeltaSet"):]
    assert "pub unsafe fn encode_batch_device(" in gpu_index
    docs = open(os.path.join(ROOT, "docs", "delta.md")).read()
    assert "nmn_deltaset_limits" in docs and "256 MiB" in docs


def test_host_born_sets_hold_their_arrays_and_a_stored_count():
    """docs/delta.md §9: only a set made on the device is without host arrays; nnz answers from the stored count on every kind"""
    arch, rows = dc.encode_inputs(65, n=70)
    lib, twin = dc.registries(65, arch, mdr=HOST)
    s = lib.encode_batch(rows, 1e-3, True)
    want = [d for d, _ in twin.encode_batch(rows, 1e-3, True)]
    assert s.host_arrays_present and s.nnz == sum(d.nnz() for d in want) == s.positions.size
    p = dc.lib_set(lib, want)
    assert p.host_arrays_present and p.nnz == s.nnz
    assert lib.encode_batch(rows[:0], 1e-3).nnz == 0


def test_search_scratch_bytes_follow_the_documented_layout():
    """docs/delta.md §8: the archetype dots nq x (K + 1) floats, the score words nq x n, and above the select kernel's k the ranked
    copy of one query's words and the sort keys (the next power of two >= max(n, 4096), 8 bytes each); each part rounded up to 256"""
    s, _, _ = sc.planted(HOST, np.arange(5000, dtype=F))

    def up(b):
        return (b + 255) // 256 * 256
    assert s.search_scratch_bytes(3, 10) == up(3 * 2 * 4) + up(3 * 5000 * 4)
    assert s.search_scratch_bytes(3, 4096) == s.search_scratch_bytes(3, 1)
    assert s.search_scratch_bytes(3, 4097) == up(3 * 2 * 4) + up(3 * 5000 * 4) + up(5000 * 4) + 8192 * 8
