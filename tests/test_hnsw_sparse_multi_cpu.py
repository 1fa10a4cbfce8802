"""nmn_hnsw_search_sparse_multi and sparse calls in the coalescer (docs/hnsw.md §14) without a GPU: the symbol is exported, declared,
bound and in the Rust FFI; the queue header carries a sparse call without learning HIP; the queue's tool drives sparse calls."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_GPU_SYMBOLS = ["nmn_hnsw_search_sparse_multi"]


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
    assert callable(GpuHnsw.search_sparse_multi)
    wrapper = open(os.path.join(ROOT, "integration", "rust", "gpu_index.rs")).read()
    assert "pub fn search_sparse_multi" in wrapper and "ffi::nmn_hnsw_search_sparse_multi" in wrapper


def test_the_signature_is_the_csr_of_search_sparse_with_the_k_and_ef_of_search_multi():
    import ctypes as C
    from neumann_amd import _capi
    res, args = _capi.SIGNATURES["nmn_hnsw_search_sparse_multi"]
    _, sparse = _capi.SIGNATURES["nmn_hnsw_search_sparse"]
    _, multi = _capi.SIGNATURES["nmn_hnsw_search_multi"]
    assert res is C.c_int32
    assert args[:5] == sparse[:5]           # handle, indptr, positions, values, nq
    assert args[5:] == multi[3:]            # k, ef, kstride, out_ids, out_scores, out_counts, stats


def test_the_queue_header_stays_free_of_hip_and_carries_sparse_calls():
    src = open(os.path.join(ROOT, "neumann_amd", "csrc", "nmn_hnsw_queue.h")).read()
    assert "hip" not in re.sub(r"//.*", "", src).lower()
    code = re.sub(r"//.*", "", src)
    assert re.search(r"struct\s+SparseQueries\s*;", code)                     # a forward declaration: the queue never looks inside
    assert re.search(r"const\s+SparseQueries\s*\*\s*sp\s*=\s*nullptr", code)   # HostWalk's sparse call


def test_the_tool_drives_sparse_calls():
    tool = open(os.path.join(ROOT, "tools", "micro", "hnsw_queue_mt.cpp")).read()
    assert re.search(r"me\.sp\s*=\s*&", tool) and "SparseQueries" in tool
    assert "-fsanitize=thread" in tool and "-fsanitize=address" in tool


def test_the_entries_go_through_the_coalescer():
    """both sparse entries build a HostWalk and hand it to the code path of nmn_hnsw_search; neither takes host_mu itself"""
    src = open(os.path.join(ROOT, "neumann_amd", "csrc", "nmn_hnsw.hip")).read()
    for name in ("nmn_hnsw_search_sparse", "nmn_hnsw_search_sparse_multi"):
        body = src[src.index(f'extern "C" nmn_status {name}('):]
        body = body[:body.index("\n}\n")]
        assert "me.sp = &sq" in body and "host_walk_call(h, me, stats)" in body, name
        assert "host_mu" not in body, name
