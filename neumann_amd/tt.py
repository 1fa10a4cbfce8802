"""Tensor-train vectors — host wrapper of `nmn_tt_*` (include/neumann_gpu.h, docs/hnsw.md §17).

`TTVector` carries what `tensor_compress::TTVector` (tensor_compress/src/tensor_train.rs:267-281) carries — a shape, the ranks and
the cores — and validates as the C entries do; `tt_reconstruct` / `tt_norm` run tt_reconstruct (401-436) and tt_norm (440-474) on the
GPU, bit for bit.  `TTConfig` and `tt_decompose` are tensor_compress's (41-126, 315-397): from a dense vector and a config to a
train, bit for bit (nmn_tt_decompose, docs/hnsw.md §21)."""
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

    @classmethod
    def _from_decompose(cls, shape, ranks, flat):
        """what nmn_tt_decompose returned: taken as it is (a two-core train may carry a rank of 0, which the entries that take
        trains refuse)"""
        t = cls.__new__(cls)
        t.shape, t.ranks, t.cores, at = list(shape), [int(r) for r in ranks], [], 0
        for k, n in enumerate(t.shape):
            size = t.ranks[k] * n * t.ranks[k + 1]
            t.cores.append(np.array(flat[at:at + size], dtype=np.float32).reshape(t.ranks[k], n, t.ranks[k + 1]))
            at += size
        return t

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


# ---- tt_dot_product, tt_cosine_similarity, tt_euclidean_distance (tensor_train.rs:480-546, 591-646), docs/hnsw.md §23 ----------
SIM_DOT, SIM_COSINE, SIM_EUCLIDEAN = 0, 1, 2
SIM_OPS = {"dot": SIM_DOT, "cosine": SIM_COSINE, "euclidean": SIM_EUCLIDEAN}
INCOMPATIBLE_SHAPES = "incompatible TT shapes for operation"   # Display of TTError::IncompatibleShapes


def _trains(x):
    return [x] if isinstance(x, TTVector) else list(x)


def tt_similarity(op, queries, targets):
    """-> f32 [nq][nt]: out[i][j] = tt_dot_product / tt_cosine_similarity / tt_euclidean_distance of (queries[i], targets[j]), bit
    for bit (nmn_tt_similarity).  op: "dot", "cosine", "euclidean" or an NMN_TT_SIM_* value.  Trains of another shape raise with the
    reference's text, as the first failing pair would."""
    op = SIM_OPS.get(op, op)
    qs, ts = _trains(queries), _trains(targets)
    if any(t.shape != qs[0].shape for t in qs + ts if qs):
        raise _bad(INCOMPATIBLE_SHAPES)
    out = np.empty((len(qs), len(ts)), dtype=np.float32)
    if not qs or not ts:
        if op not in (SIM_DOT, SIM_COSINE, SIM_EUCLIDEAN):
            raise _bad("TT similarity: unknown op")
        return out
    sq, rq, oq, cq = pack(qs)
    st, rt, ot, ct = pack(ts)
    _capi.check(_capi.load().nmn_tt_similarity(int(op), _p(sq), sq.size, _p(rq), _p(oq), _p(cq), len(qs), _p(st), st.size, _p(rt), _p(ot),
                                               _p(ct), len(ts), _p(out)))
    return out


def tt_self_dot(tts):
    """-> f32 [n]: tt_dot_product(t, t) of every train, the value tt_norm takes the square root of (nmn_tt_self_dot)"""
    shape, ranks, off, cores = pack(tts)
    out = np.empty(ranks.shape[0], dtype=np.float32)
    _capi.check(_capi.load().nmn_tt_self_dot(_p(shape), shape.size, _p(ranks), _p(off), _p(cores), ranks.shape[0], _p(out)))
    return out


def tt_dot_product(a, b):
    """tt_dot_product (tensor_train.rs:480-516) -> float"""
    return float(tt_similarity(SIM_DOT, a, b)[0, 0])


def tt_cosine_similarity(a, b):
    """tt_cosine_similarity (522-532) -> float"""
    return float(tt_similarity(SIM_COSINE, a, b)[0, 0])


def tt_euclidean_distance(a, b):
    """tt_euclidean_distance (539-546) -> float"""
    return float(tt_similarity(SIM_EUCLIDEAN, a, b)[0, 0])


def tt_dot_product_batch(query, targets):
    """tt_dot_product_batch (614-623) -> f32 [len(targets)]; one target of another shape fails the whole call"""
    return tt_similarity(SIM_DOT, query, list(targets))[0]


def tt_cosine_similarity_batch(query, targets):
    """tt_cosine_similarity_batch (591-606)"""
    return tt_similarity(SIM_COSINE, query, list(targets))[0]


def tt_euclidean_distance_batch(query, targets):
    """tt_euclidean_distance_batch (631-646)"""
    return tt_similarity(SIM_EUCLIDEAN, query, list(targets))[0]


class TTDeviceSet:
    """n trains of one shape in device memory (torch tensors), as nmn_tt_decompose_device leaves them: ranks int32 [n][d + 1], cores
    f32 [n * stride], train i at core_off[i] (int64 [n + 1]) or at i * stride; status int32 [n] or None."""

    def __init__(self, ranks, cores, stride, core_off=None, status=None):
        self.ranks, self.cores, self.stride, self.core_off, self.status = ranks, cores, int(stride), core_off, status
        self.n = int(ranks.shape[0])
        if cores.numel() < self.n * self.stride:
            raise _bad("TT similarity: cores must hold n * stride floats")

    def _args(self):
        ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None   # noqa: E731
        return ptr(self.ranks), ptr(self.core_off), ptr(self.cores), self.stride, ptr(self.status), self.n


def _stream(stream):
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream if stream is None else stream)


def tt_self_dot_device(shape, trains, out=None, stream=None):
    """nmn_tt_self_dot_device: enqueued on the stream, not waited for -> f32 tensor [n] on the device"""
    import torch
    sh = np.asarray(shape, dtype=np.uint32)
    if out is None:
        out = torch.empty(trains.n, dtype=torch.float32, device=trains.cores.device)
    _capi.check(_capi.load().nmn_tt_self_dot_device(_p(sh), sh.size, *trains._args(), C.c_void_p(out.data_ptr()), _stream(stream)))
    return out


def tt_similarity_device(op, shape, queries, targets, self_q=None, self_t=None, out=None, stream=None):
    """nmn_tt_similarity_device on two TTDeviceSets: enqueued on the stream, not waited for -> f32 tensor [nq][nt] on the device.
    self_q / self_t: what tt_self_dot_device returned for the sets (cosine and Euclidean need both)."""
    import torch
    op = SIM_OPS.get(op, op)
    sh = np.asarray(shape, dtype=np.uint32)
    if out is None:
        out = torch.empty((queries.n, targets.n), dtype=torch.float32, device=queries.cores.device)
    ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None   # noqa: E731
    _capi.check(_capi.load().nmn_tt_similarity_device(int(op), _p(sh), sh.size, *queries._args(), *targets._args(), ptr(self_q),
                                                      ptr(self_t), C.c_void_p(out.data_ptr()), _stream(stream)))
    return out


PRESETS = {"for_dim": 0, "high_compression": 1, "high_accuracy": 2}


class TTConfig:
    """tensor_compress::TTConfig (tensor_train.rs:41-49): the shape a vector is folded into, the largest TT-rank, and the relative
    tolerance at which the SVD of a step stops."""

    def __init__(self, shape, max_rank=8, tolerance=1e-4):
        self.shape = [int(x) for x in shape]
        self.max_rank = int(max_rank)
        self.tolerance = float(np.float32(tolerance))

    def __repr__(self):
        return f"TTConfig(shape={self.shape}, max_rank={self.max_rank}, tolerance={self.tolerance})"

    def __eq__(self, other):
        return isinstance(other, TTConfig) and (self.shape, self.max_rank, self.tolerance) == (other.shape, other.max_rank, other.tolerance)

    @classmethod
    def _preset(cls, dim, preset):
        shape = (C.c_uint32 * 8)()
        n, r, t = C.c_uint32(), C.c_uint32(), C.c_float()
        _capi.check(_capi.load().nmn_tt_config_for_dim(int(dim), PRESETS[preset], shape, C.byref(n), C.byref(r), C.byref(t)))
        return cls(list(shape[:n.value]), r.value, t.value)

    @classmethod
    def for_dim(cls, dim):
        """TTConfig::for_dim (77-89): optimal_shape(dim), max_rank 8, tolerance 1e-4"""
        return cls._preset(dim, "for_dim")

    @classmethod
    def high_compression(cls, dim):
        """TTConfig::high_compression (95-107): max_rank 4, tolerance 1e-2"""
        return cls._preset(dim, "high_compression")

    @classmethod
    def high_accuracy(cls, dim):
        """TTConfig::high_accuracy (113-125): max_rank 16, tolerance 1e-6"""
        return cls._preset(dim, "high_accuracy")

    def validate(self):
        """TTConfig::validate (56-70), its Display texts; tt_decompose itself does not call it"""
        if not self.shape:
            raise _bad("invalid shape: empty shape")
        if 0 in self.shape:
            raise _bad("invalid shape: shape contains zero")
        if self.max_rank < 1:
            raise _bad("invalid TT-rank: must be >= 1")
        t = self.tolerance
        if not (t > 0.0 and t <= 1.0):
            raise _bad(f"invalid tolerance: {t} (must be 0 < tol <= 1)")

    @property
    def max_storage(self):
        """the slot of one train in floats (nmn_tt_max_storage)"""
        sh = np.asarray(self.shape, dtype=np.uint32)
        return int(_capi.load().nmn_tt_max_storage(_p(sh), sh.size, max(self.max_rank, 0)))

    def _c(self):
        if self.max_rank < 0 or any(n < 0 for n in self.shape):
            raise _bad("invalid TT-rank: must be >= 1" if self.max_rank < 0 else "invalid shape: negative mode")
        return np.asarray(self.shape, dtype=np.uint32), self.max_rank, C.c_float(self.tolerance)


class TTDecomposeError(_capi.NeumannGpuError):
    """one vector's Err of tt_decompose; `kind` is the Debug form of the reference's TTError"""

    def __init__(self, kind, text):
        super().__init__(_capi.ERR_INVALID_ARGUMENT, text)
        self.kind = kind


def decompose_limits():
    """(max_cores, max_rank, max_dim, max_lds_floats): what the device path of tt_decompose serves (nmn_tt_decompose_limits); a
    config is served there when `decompose_lds_floats` is at most max_lds_floats"""
    v = [C.c_uint32() for _ in range(4)]
    _capi.check(_capi.load().nmn_tt_decompose_limits(*[C.byref(x) for x in v]))
    return tuple(int(x.value) for x in v)


def decompose_lds_floats(config):
    """the LDS floats `config` needs on the device, None when it is above the limits (nmn_tt_decompose_lds_floats)"""
    sh, r, _ = config._c()
    v = int(_capi.load().nmn_tt_decompose_lds_floats(_p(sh), sh.size, r))
    return None if v == 2 ** 64 - 1 else v


def tt_decompose_raw(vectors, config, want_cores=True):
    """nmn_tt_decompose as it is -> (status u32 [n], ranks u32 [n][d + 1], core_off u64 [n + 1], cores f32)"""
    v = np.ascontiguousarray(vectors, dtype=np.float32)
    if v.ndim == 1:
        v = v[None, :]
    sh, r, tol = config._c()
    n, dim = v.shape
    status = np.zeros(n, dtype=np.uint32)
    ranks = np.zeros((n, sh.size + 1), dtype=np.uint32)
    off = np.zeros(n + 1, dtype=np.uint64)
    cap = n * int(_capi.load().nmn_tt_max_storage(_p(sh), sh.size, r)) if want_cores else 0
    cores = np.zeros(max(cap, 1), dtype=np.float32)
    _capi.check(_capi.load().nmn_tt_decompose(_p(v), n, dim, _p(sh), sh.size, r, tol, _p(status), _p(ranks), _p(off),
                                              _p(cores) if want_cores else None, cap))
    return status, ranks, off, cores[:int(off[n])]


def tt_decompose(vectors, config, return_status=False):
    """tt_decompose (tensor_train.rs:315-397) of one vector [dim] or several [n][dim] under `config`, bit for bit -> a list of
    TTVector.  A vector whose decomposition is an Err (Decompose(EmptyMatrix)) raises TTDecomposeError; with return_status=True the
    list holds that error in the vector's slot instead.  An empty vector, a shape whose product is not the dimension and
    max_rank < 1 refuse the call with the reference's text."""
    status, ranks, off, cores = tt_decompose_raw(vectors, config)
    out = []
    for q in range(status.size):
        if status[q] == 0:
            out.append(TTVector._from_decompose(config.shape, ranks[q], cores[int(off[q]):int(off[q + 1])]))
            continue
        err = TTDecomposeError("Decompose(EmptyMatrix)", f"TT: vector {q}: decomposition error: empty matrix")
        if not return_status:
            raise err
        out.append(err)
    return out
