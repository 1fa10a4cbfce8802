"""The device-buffer sparse entries (docs/hnsw.md §22) without a GPU: nmn_sparse_canonicalise_device,
nmn_hnsw_search_sparse_device and nmn_hnsw_cache_search_sparse_device are declared, bound and exported, and refuse a max_nnz above
4096 and null arguments before they touch a device."""
import ctypes as C
import os
import re

import pytest

from neumann_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("nmn_sparse_canonicalise_device", "nmn_hnsw_search_sparse_device", "nmn_hnsw_cache_search_sparse_device")
PTR = C.c_void_p(64)  # never dereferenced: every call below is refused before a device is touched


def _err():
    return _capi.load().nmn_last_error().decode()


def _canon(dim=8, indptr=PTR, pos=PTR, val=PTR, nq=1, nnz=4, max_nnz=0, off=PTR, ent=PTR, mag=PTR, status=PTR):
    return _capi.load().nmn_sparse_canonicalise_device(dim, indptr, pos, val, nq, nnz, max_nnz, off, ent, mag, None, None, status, -1, None)


@pytest.mark.parametrize("name", NEW)
def test_declared_bound_and_exported(name):
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "neumann_gpu.h")).read(), flags=re.S)
    assert re.search(rf"\bnmn_status {name}\s*\(", header), "not declared in include/neumann_gpu.h"
    assert name in _capi.SIGNATURES
    ffi = open(os.path.join(ROOT, "integration", "rust", "ffi.rs")).read()
    assert len(re.findall(rf"pub fn {name}\(", ffi)) == 1
    assert hasattr(_capi.load(), name), "not exported by the built library"
    # one ctypes argument per C parameter
    params = re.search(rf"\b{name}\s*\((.*?)\);", header, flags=re.S).group(1)
    assert len(_capi.SIGNATURES[name][1]) == len(params.split(","))


def test_canonicalise_refuses_max_nnz_above_4096():
    assert _canon(max_nnz=4097) == _capi.ERR_INVALID_ARGUMENT
    assert "max_nnz" in _err() and "4096" in _err()
    assert _canon(dim=8192, max_nnz=2**32 - 1) == _capi.ERR_INVALID_ARGUMENT


def test_canonicalise_refuses_bad_dimensions_and_nulls():
    assert _canon(dim=0) != 0
    assert _canon(dim=8193) == _capi.ERR_CONFIGURATION
    for kw in ("indptr", "pos", "val", "off", "ent", "mag", "status"):
        assert _canon(**{kw: None}) == _capi.ERR_INVALID_ARGUMENT, kw
        assert "null" in _err()
    assert _canon(nq=0, indptr=None, off=None) == 0  # nothing to do, nothing looked at


def test_search_entries_refuse_without_a_handle():
    lib = _capi.load()
    m = _capi.XMetric()
    # max_nnz is checked first, so its text comes even with no handle
    assert lib.nmn_hnsw_search_sparse_device(None, PTR, PTR, PTR, 1, 4, 5000, 3, 0, PTR, PTR, PTR, None, None) == _capi.ERR_INVALID_ARGUMENT
    assert "max_nnz" in _err()
    assert lib.nmn_hnsw_cache_search_sparse_device(None, PTR, PTR, PTR, 1, 4, 5000, 3, 0.5, C.byref(m), PTR, PTR, PTR, None,
                                                   None) == _capi.ERR_INVALID_ARGUMENT
    assert "max_nnz" in _err()
    assert lib.nmn_hnsw_search_sparse_device(None, PTR, PTR, PTR, 1, 4, 0, 3, 0, PTR, PTR, PTR, None, None) == _capi.ERR_INVALID_ARGUMENT
    assert "null" in _err()
    assert lib.nmn_hnsw_cache_search_sparse_device(None, PTR, PTR, PTR, 1, 4, 0, 3, 0.5, C.byref(m), PTR, PTR, PTR, None,
                                                   None) == _capi.ERR_INVALID_ARGUMENT
    assert "null" in _err()
