"""nmn_hnsw_search_metric_multi (docs/hnsw.md §12) without a GPU: the symbol is exported, declared, bound and in the Rust FFI, and
the coalescer's queue keeps a call marked `alone` in a batch of its own."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_GPU_SYMBOLS = ["nmn_hnsw_search_metric_multi"]


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
    assert callable(GpuHnsw.search_metric_multi)


def test_the_queue_header_stays_free_of_hip_and_knows_lone_calls():
    src = open(os.path.join(ROOT, "neumann_amd", "csrc", "nmn_hnsw_queue.h")).read()
    assert "hip" not in re.sub(r"//.*", "", src).lower()
    assert "alone" in src and "kShareCandMax" in src
    tool = open(os.path.join(ROOT, "tools", "micro", "hnsw_queue_mt.cpp")).read()
    assert "alone" in tool
