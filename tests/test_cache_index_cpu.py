"""tests/_cache_index_oracle.py held to hand-derived answers (docs/hnsw.md §16), the frozen tests/golden/cache_index_small.npz held to
the oracle, and the plumbing of nmn_hnsw_cache_search* / nmn_hnsw_set_node_mask without a GPU: symbols exported, declared, bound and in
the Rust FFI; the queue header carries a cache call without learning HIP; the queue's tool drives cache calls."""
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from tests import _cache_index_oracle as co
from tests import _hnsw_mixed_oracle as mo
from tests import _hnsw_oracle as ho
from tests import _xmetric_oracle as xo

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "cache_index_small.npz")
NEW_GPU_SYMBOLS = ["nmn_hnsw_set_node_mask", "nmn_hnsw_node_live", "nmn_hnsw_cache_search", "nmn_hnsw_cache_search_sparse",
                   "nmn_hnsw_cache_search_device"]
NINE = [xo.Metric(k) for k in range(8)] + [xo.Metric(xo.COMPOSITE, xo.GeometricConfig.default())]


# ---- duplicated positions: a = {(2, 1.0), (2, 3.0)}, b = {(2, 5.0)}, by hand ------------------------------------------------------
def _ab():
    a = co.Entries(mo.SparseVector.from_parts(4, [2, 2], [1.0, 3.0]))
    b = co.Entries(mo.SparseVector.from_parts(4, [2], [5.0]))
    a_dense = xo.Sparse(mo.SparseVector.from_parts(4, [2, 2], [1.0, 3.0]).to_dense())
    return a, b, a_dense


def test_try_from_parts_keeps_duplicates_in_input_order():
    a, _, a_dense = _ab()
    assert a.positions == [2, 2] and a.values == [1.0, 3.0]
    assert a_dense.positions == [2] and a_dense.values == [3.0]      # to_dense: the last of a position wins


@pytest.mark.parametrize("kind, stored, densified", [
    (xo.JACCARD, 0.5, 1.0),            # one pair of 2 + 1 - 1 positions
    (xo.OVERLAP, 1.0, None),           # 1 / min(2, 1)
    (xo.WEIGHTED_JACCARD, 0.125, None),  # (min(1, 5) + min(3, 0)) / (max(1, 5) + max(3, 0)) = 1 / 8
    (xo.EUCLIDEAN, 5.0, 2.0),          # sqrt((1 - 5)^2 + 3^2); sqrt((3 - 5)^2)
    (xo.MANHATTAN, 7.0, None),         # |1 - 5| + |3|
])
def test_duplicate_table(kind, stored, densified):
    a, b, a_dense = _ab()
    m = xo.Metric(kind)
    assert float(xo.compute(m, a, b)) == stored
    if densified is not None:
        assert float(xo.compute(m, a_dense, b)) == densified


def test_duplicate_table_dot_and_cosine():
    a, b, a_dense = _ab()
    assert xo.dot_f64(a, b) == 5.0 and xo.dot_f64(a_dense, b) == 15.0   # the first duplicate pairs, the second finds b exhausted
    want = F(5.0 / (math.sqrt(10.0) * 5.0))
    assert xo.compute(xo.Metric(xo.COSINE), a, b).tobytes() == want.tobytes()
    assert float(xo.compute(xo.Metric(xo.COSINE), a_dense, b)) == 1.0


# ---- the candidate rule ------------------------------------------------------------------------------------------------------------
def test_candidate_rule():
    assert [co.candidate_count(k) for k in (0, 1, 3, 4, 10)] == [10, 10, 10, 12, 30]
    assert co.candidate_count(1 << 63) == (1 << 64) - 1


def _eye_index(n=16, dim=16):
    """rows e_i scaled so that the walk's order from e_0 + small is unambiguous"""
    c = co.CacheIndex(dim)
    rng = np.random.default_rng(3)
    rows = rng.standard_normal((n, dim)).astype(F)
    for i in range(n):
        c.insert(f"k{i}", rows[i])
    return c, rows


def test_candidates_are_3k_and_min_with_len():
    c, rows = _eye_index(16)
    seen = {}
    walk = c.index.search

    def spy(q, k):
        seen["k"] = k
        return walk(q, k)
    c.index.search = spy
    m = xo.Metric(xo.COSINE)
    for k, want in ((1, 10), (3, 10), (4, 12)):
        res = c.search_with_metric(rows[0], k, -math.inf, m)
        assert seen["k"] == want and len(res) == k
    assert len(c.search_with_metric(rows[0], 10, -math.inf, m)) == 10     # c = 30, served as min(30, 16) = 16, truncated to 10
    assert len(c.search_with_metric(rows[0], 16, -math.inf, m)) == 16
    assert len(c.search_with_metric(rows[0], 100, -math.inf, m)) == 16


def test_threshold_equality_nan_and_k0():
    c, rows = _eye_index(12)
    m = xo.Metric(xo.EUCLIDEAN)
    full = c.search_with_metric(rows[1], 5, -math.inf, m)
    sims = [s for _, s in full]
    assert sims == sorted(sims, reverse=True) and full[0] == ("k1", F(1.0))
    cut = sims[2]
    kept = c.search_with_metric(rows[1], 5, cut, m)            # a similarity exactly equal to the threshold passes
    assert kept == full[:3]
    above = np.nextafter(cut, F(2.0), dtype=F)
    assert c.search_with_metric(rows[1], 5, above, m) == full[:2]
    assert c.search_with_metric(rows[1], 5, math.nan, m) == []  # nothing is >= NaN
    assert c.search_with_metric(rows[1], 5, math.inf, m) == []
    assert c.search_with_metric(rows[1], 0, -math.inf, m) == []  # k == 0: truncated to nothing, not an error
    with pytest.raises(co.DimensionMismatch):
        c.search_with_metric(rows[1][:5], 1, 0.0, m)
    assert co.CacheIndex(12).search_with_metric(rows[1][:12], 3, -math.inf, m) == []   # an empty index


def test_the_walk_uses_the_indexs_own_hnsw_metric():
    cfg = ho.HNSWConfig().with_distance_metric(ho.EUCLIDEAN)
    c = co.CacheIndex(4, cfg)
    c.insert("far-aligned", [10.0, 0.0, 0.0, 0.0])
    c.insert("near", [1.0, 1.0, 0.0, 0.0])
    assert [n for n, _ in c.index.search(np.array([1.0, 0.0, 0.0, 0.0], dtype=F), 2)] == [1, 0]   # Euclidean order, not cosine
    res = c.search_with_metric([1.0, 0.0, 0.0, 0.0], 2, -1.0, xo.Metric(xo.COSINE))
    assert [k for k, _ in res] == ["far-aligned", "near"]     # ... and the re-rank is the asked metric's


# ---- the key maps' surprises -------------------------------------------------------------------------------------------------------
def test_reinsert_answers_twice_and_remove_leaves_the_orphan():
    c = co.CacheIndex(3)
    assert c.insert("a", [1.0, 0.0, 0.0]) == 0
    assert c.insert("a", [0.9, 0.1, 0.0]) == 1
    assert len(c) == 1 and c.keys() == ["a"]
    res = c.search_with_metric([1.0, 0.0, 0.0], 5, -1.0, xo.Metric(xo.COSINE))
    assert [k for k, _ in res] == ["a", "a"]
    assert c.remove("a") and not c.contains("a") and len(c) == 0 and c.is_empty()
    res = c.search_with_metric([1.0, 0.0, 0.0], 5, -1.0, xo.Metric(xo.COSINE))
    assert [k for k, _ in res] == ["a"] and res[0][1] == F(1.0)   # node 0, orphaned by the re-insert, still answers
    assert not c.remove("a")
    assert c.get_embedding("a") is None


def test_insert_auto_at_exactly_the_threshold():
    c = co.CacheIndex(4)
    v = [1.0, 0.0, 2.0, 0.0]                       # sparsity = 1 - 2/4 = 0.5 exactly
    c.insert_auto("s", v, 0.5)
    c.insert_auto("d", v, np.nextafter(F(0.5), F(1.0)))
    assert c.get_embedding("s")[0] == "sparse" and c.get_embedding("d")[0] == "dense"
    c.insert_auto("n", v, math.nan)
    assert c.get_embedding("n")[0] == "dense"      # nothing is >= NaN
    assert c.memory_stats()["sparse_count"] == 1


def test_clear_restarts_ids_and_the_level_generator():
    c = co.CacheIndex(3)
    rows = np.random.default_rng(1).standard_normal((30, 3)).astype(F)
    for i, r in enumerate(rows):
        c.insert(f"k{i}", r)
    levels = list(c.index.levels)
    c.clear()
    assert len(c) == 0 and c.keys() == [] and c.search([1.0, 0.0, 0.0], 3, -1.0) == []
    for i, r in enumerate(rows):
        assert c.insert(f"k{i}", r) == i
    assert c.index.levels == levels and levels[0] == ho.HNSWIndex().random_level()


# ---- the frozen golden ---------------------------------------------------------------------------------------------------------------
_GOLDEN_INDEX = {}


def golden_index(g):
    """the oracle CacheIndex the golden file describes (built once: the tests below only search it)"""
    if "c" in _GOLDEN_INDEX:
        return _GOLDEN_INDEX["c"]
    nodes = iter(mo.vectors_from_csr(g["rows"].shape[1], g["node_indptr"], g["node_pos"], g["node_val"]))
    c = co.CacheIndex(g["rows"].shape[1])
    for i in range(g["rows"].shape[0]):
        key = f"k{g['keys'][i]}"
        if g["sparse_mask"][i]:
            c.insert_sparse(key, next(nodes))
        else:
            c.insert(key, g["rows"][i])
    for k in g["removed"]:
        assert c.remove(f"k{k}")
    _GOLDEN_INDEX["c"] = c
    return c


def test_golden_is_what_the_oracle_answers():
    g = np.load(GOLDEN)
    c = golden_index(g)
    n = g["rows"].shape[0]
    assert [i in c.node_to_key for i in range(n)] == g["live"].tolist() and len(c) == 320
    assert np.array_equal(c.index.to_dense_rows(), g["rows"])
    sqs = mo.vectors_from_csr(g["rows"].shape[1], g["sq_indptr"], g["sq_pos"], g["sq_val"])
    assert sum(s.has_duplicates() for s in sqs) == 16 and sum(s.has_duplicates() for s in c.index.sparse.values()) == 20
    live = c.node_to_key.__contains__
    ks = (1, 4, 10)
    # sixteen of the 64 queries of each form, spread over the file; the odd ones' sparse forms hold a duplicated position
    for qi in list(range(0, 64, 8)) + list(range(1, 64, 8)):
        walks = {cc: ([n for n, _ in c.index.search(g["dense_queries"][qi], cc)],
                      [n for n, _ in c.index.search_sparse_with_ef(sqs[qi], cc, c.index.config.ef_search)]) for cc in (10, 12, 20, 30)}
        for form, fi in (("dense", 0), ("sparse", 1)):
            ent = xo.Sparse(g["dense_queries"][qi]) if form == "dense" else co.Entries(sqs[qi])
            twin = ent if form == "dense" else xo.Sparse(sqs[qi].to_dense())
            for mi, metric in enumerate(NINE):
                thr = g[f"{form}_thresholds"][mi, qi]
                for ki, k in enumerate(ks):
                    res = co.rescore(c.index, live, walks[co.candidate_count(k)][fi], ent, k, thr, metric)
                    cnt = int(g[f"{form}_k{k}_counts"][mi, qi])
                    assert len(res) == cnt, (form, qi, metric, k)
                    assert [nid for nid, _ in res] == g[f"{form}_k{k}_ids"][mi, qi, :cnt].tolist()
                    assert np.array([s for _, s in res], dtype=F).tobytes() == g[f"{form}_k{k}_sims"][mi, qi, :cnt].tobytes()
                    # the stored flag "differs from the re-rank of the to_dense() forms under max(2k, 10)", recomputed
                    alt = co.rescore_densified(c.index, live, walks[xo.candidate_count(k)][fi], twin, k, thr, metric)
                    differs = [(n, F(x).tobytes()) for n, x in res] != [(n, F(x).tobytes()) for n, x in alt]
                    assert differs == bool(g[f"{form}_differ"][mi, qi, ki]), (form, qi, metric, k)
    n_differ = int(g["dense_differ"].sum() + g["sparse_differ"].sum())
    assert n_differ == int(g["n_differ"]) and 4 * n_differ >= 9 * 128 * 3


def test_search_nodes_is_the_walk_and_the_rescore():
    """(the golden check above feeds rescore with the walk's candidates itself; search_nodes must be exactly that)"""
    g = np.load(GOLDEN)
    c = golden_index(g)
    live = c.node_to_key.__contains__
    sq = mo.vectors_from_csr(g["rows"].shape[1], g["sq_indptr"], g["sq_pos"], g["sq_val"])[5]
    q = g["dense_queries"][3]
    m = NINE[5]
    assert co.search_nodes(c.index, live, q, 4, 0.1, m) == co.rescore(c.index, live, [n for n, _ in c.index.search(q, 12)], xo.Sparse(q), 4, 0.1, m)
    assert co.search_nodes_sparse(c.index, live, sq, 4, 0.1, m) == co.rescore(
        c.index, live, [n for n, _ in c.index.search_sparse_with_ef(sq, 12, c.index.config.ef_search)], co.Entries(sq), 4, 0.1, m)


# ---- plumbing ------------------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_exported_declared_and_bound():
    from neumann_amd import _capi
    lib = _capi.load()
    gpu_h = open(os.path.join(ROOT, "include", "neumann_gpu.h")).read()
    ffi = open(os.path.join(ROOT, "integration", "rust", "ffi.rs")).read()
    for name in NEW_GPU_SYMBOLS:
        assert hasattr(lib, name), name
        assert re.search(rf"\b{name}\s*\(", gpu_h), name
        assert re.search(rf"pub fn {name}\(", ffi), name
        assert name in _capi.SIGNATURES
    from neumann_amd import GpuHnsw
    for m in ("cache_search", "cache_search_sparse", "cache_search_device", "set_node_mask", "node_live"):
        assert callable(getattr(GpuHnsw, m)), m
    wrapper = open(os.path.join(ROOT, "integration", "rust", "gpu_index.rs")).read()
    for m in ("cache_search", "cache_search_sparse", "set_node_mask", "node_live"):
        assert f"pub fn {m}(" in wrapper and f"ffi::nmn_hnsw_{m}(" in wrapper, m
    assert "does NOT store the\n * mask" in gpu_h or "does NOT store the mask" in gpu_h


def test_key_layer_symbols_are_exported_declared_and_bound():
    from neumann_amd import CacheIndex, _capi, cache_index
    lib = _capi.load()
    src = open(os.path.join(ROOT, "include", "neumann_cache.h")).read()
    declared = sorted(set(re.findall(r"\b(nmn_cache_index_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", src, flags=re.S))))
    for fn in ("create", "destroy", "insert", "insert_sparse", "insert_auto", "search", "search_with_metric", "search_sparse",
               "search_sparse_with_metric", "remove", "contains", "len", "dimension", "keys", "clear", "memory_stats", "get_embedding",
               "last_error"):
        assert f"nmn_cache_index_{fn}" in declared, fn
    for name in declared:
        assert hasattr(lib, name), f"{name} declared in include/neumann_cache.h but not exported"
    assert set(declared) == set(cache_index.SIGNATURES), set(declared) ^ set(cache_index.SIGNATURES)
    from neumann_amd import build
    assert "nmn_cache_index.cpp" in build.SOURCES
    for m in ("insert", "insert_sparse", "insert_auto", "search", "search_with_metric", "search_sparse", "search_sparse_with_metric",
              "remove", "contains", "keys", "clear", "memory_stats", "get_embedding"):
        assert callable(getattr(CacheIndex, m)), m


def test_rust_ffi_is_current():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_rust_ffi.py"), "--check"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr


def test_signatures_are_search_metrics_with_a_threshold():
    import ctypes as C
    from neumann_amd import _capi
    _, metric = _capi.SIGNATURES["nmn_hnsw_search_metric"]
    _, cache = _capi.SIGNATURES["nmn_hnsw_cache_search"]
    assert cache == metric[:4] + [C.c_float] + metric[4:]
    _, metric_dev = _capi.SIGNATURES["nmn_hnsw_search_metric_device"]
    _, cache_dev = _capi.SIGNATURES["nmn_hnsw_cache_search_device"]
    assert cache_dev == metric_dev[:4] + [C.c_float] + metric_dev[4:]
    _, sparse = _capi.SIGNATURES["nmn_hnsw_search_sparse"]
    _, cache_sp = _capi.SIGNATURES["nmn_hnsw_cache_search_sparse"]
    assert cache_sp[:6] == sparse[:6] and cache_sp[6:8] == [C.c_float, C.POINTER(_capi.XMetric)] and cache_sp[8:] == sparse[7:]


def test_the_queue_header_compiles_without_hip_and_carries_cache_calls(tmp_path):
    src = open(os.path.join(ROOT, "neumann_amd", "csrc", "nmn_hnsw_queue.h")).read()
    code = re.sub(r"//.*", "", src)
    assert "hip" not in code.lower()
    assert re.search(r"bool\s+filter\s*=\s*false", code) and re.search(r"float\s+threshold\s*=\s*0", code)
    prog = tmp_path / "q.cpp"
    prog.write_text('#include "nmn_hnsw_queue.h"\n'
                    "int main() { nmn::HostWalk w; w.filter = true; w.threshold = 0.9f; return w.filter && w.threshold > 0.0f ? 0 : 1; }\n")
    r = subprocess.run(["c++", "-std=c++17", "-fsyntax-only", "-I", os.path.join(ROOT, "include"),
                        "-I", os.path.join(ROOT, "neumann_amd", "csrc"), str(prog)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_the_tool_drives_cache_calls():
    tool = open(os.path.join(ROOT, "tools", "micro", "hnsw_queue_mt.cpp")).read()
    assert re.search(r"me\.filter\s*=\s*true", tool) and re.search(r"me\.threshold\s*=", tool)
    assert re.search(r"REQUIRE\(r->threshold\s*==", tool) and "r->filter" in tool
    assert "-fsanitize=thread" in tool and "-fsanitize=address" in tool


def test_the_host_entry_goes_through_the_coalescer():
    src = open(os.path.join(ROOT, "neumann_amd", "csrc", "nmn_hnsw.hip")).read()
    body = src[src.index('extern "C" nmn_status nmn_hnsw_cache_search('):]
    body = body[:body.index("\n}\n")]
    assert "me.filter = true" in body and "me.threshold = threshold" in body and "metric_walk_call(h, me, stats)" in body
    assert "host_mu" not in body
