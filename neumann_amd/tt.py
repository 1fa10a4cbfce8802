"""Tensor-train vectors — host wrapper of `nmn_tt_*` (include/neumann_gpu.h, docs/hnsw.md §17).

`TTVector` carries what `tensor_compress::TTVector` (tensor_compress/src/tensor_train.rs:267-281) carries — a shape, the ranks and
the cores — and validates as the C entries do; `tt_reconstruct` / `tt_norm` run tt_reconstruct (401-436) and tt_norm (440-474) on the
GPU, bit for bit.  Decomposing a vector (tt_decompose, a truncated SVD) is the caller's: this module takes cores."""
import ctypes as C

import numpy as np

from . import _capi


def limits():
    """(max_cores, max_rank, max_storage, max_level): what the device path prepares in LDS (nmn_tt_limits)"""
    v = [C.c_uint32() for _ in range(4)]
    _capi.check(_capi.load().nmn_tt_limits(*[C.byref(x) for x in v]))
    return tuple(int(x.value) for x in v)


def _bad(text):
    return _capi.NeumannGpuError(_capi.ERR_INVALID_ARGUMENT, text)


class TTVector:
    """shape [n_1 .. n_d], ranks [1, r_1 .. r_{d-1}, 1], cores: d arrays, core k of ranks[k] * shape[k] * ranks[k + 1] floats in
    TTCore::get's order (tensor_train.rs:240-243)."""

    def __init__(self, shape, ranks, cores):
        self.shape = [int(x) for x in shape]
        self.ranks = [int(x) for x in ranks]
        d = len(self.shape)
        if not 1 <= d <= 8:
            raise _bad("TT: n_cores must be 1..8")
        if any(n < 1 for n in self.shape):
            raise _bad("TT: every mode of the shape must be >= 1")
        if len(self.ranks) != d + 1 or len(cores) != d:
            raise _bad("TT: ranks is [n_cores + 1], cores is [n_cores]")
        if self.ranks[0] != 1 or self.ranks[-1] != 1:
            raise _bad("TT: ranks[0] and ranks[n_cores] must be 1")
        if any(r < 1 for r in self.ranks):
            raise _bad("TT: every rank must be >= 1")
        self.cores = []
        for k, c in enumerate(cores):
            a = np.ascontiguousarray(c, dtype=np.float32)
            if a.size != self.ranks[k] * self.shape[k] * self.ranks[k + 1]:
                raise _bad(f"TT: core {k} must hold ranks[k] * shape[k] * ranks[k + 1] floats")
            self.cores.append(a.reshape(self.ranks[k], self.shape[k], self.ranks[k + 1]))

    @property
    def dim(self):
        return int(np.prod(self.shape, dtype=np.int64))

    @property
    def storage_size(self):
        return sum(c.size for c in self.cores)

    def flat(self):
        return np.concatenate([c.reshape(-1) for c in self.cores])


def pack(tts):
    """one or several TTVectors of ONE shape -> (shape u32, ranks u32 [nq][d + 1], core_off u64 [nq + 1], cores f32)"""
    if isinstance(tts, TTVector):
        tts = [tts]
    tts = list(tts)
    if not tts:
        raise _bad("TT: no trains")
    for t in tts:
        if t.shape != tts[0].shape:
            raise _bad("TT: the trains of one call share one shape")
    shape = np.asarray(tts[0].shape, dtype=np.uint32)
    ranks = np.ascontiguousarray([t.ranks for t in tts], dtype=np.uint32)
    flats = [t.flat() for t in tts]
    off = np.zeros(len(tts) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([f.size for f in flats])
    return shape, ranks, off, np.ascontiguousarray(np.concatenate(flats), dtype=np.float32)


def _p(a):
    return C.c_void_p(a.ctypes.data)


def tt_reconstruct(tts):
    """-> f32 [nq][dim] (nmn_tt_reconstruct)"""
    shape, ranks, off, cores = pack(tts)
    nq = ranks.shape[0]
    out = np.empty((nq, int(np.prod(shape, dtype=np.int64))), dtype=np.float32)
    _capi.check(_capi.load().nmn_tt_reconstruct(_p(shape), shape.size, _p(ranks), _p(off), _p(cores), nq, _p(out)))
    return out


def tt_norm(tts):
    """-> f32 [nq], the raw norms (nmn_tt_norm)"""
    shape, ranks, off, cores = pack(tts)
    nq = ranks.shape[0]
    out = np.empty(nq, dtype=np.float32)
    _capi.check(_capi.load().nmn_tt_norm(_p(shape), shape.size, _p(ranks), _p(off), _p(cores), nq, _p(out)))
    return out
