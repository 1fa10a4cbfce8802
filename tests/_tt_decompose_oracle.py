"""numpy f32 twin of tt_decompose (tensor_compress/src/tensor_train.rs:315-397) and of what it calls in
tensor_compress/src/decompose.rs (matmul 197-216, dot/norm/normalize 220-239, Lcg 242-268, gaussian_matrix 271-294,
qr_orthonormalize 298-340, power_iteration 344-387, svd_truncated 398-466, svd_power_iteration 470-550, frobenius_norm 76-78,
left_unfold_for_tt 559-566), written from the Rust (docs/hnsw.md §21).  Every product and every add is one f32 operation; a chain is
never split.  It is vectorised only across outputs the reference computes independently: the rows of u, the columns of v, the
elements of a deflation, the outputs of a matmul, the elements of a Gram-Schmidt update.  logf, cosf and sinf are libm's."""
import ctypes
import math

import numpy as np

F = np.float32
NEG0 = F(-0.0)
EPS = F(1e-10)
OK, EMPTY_MATRIX = 0, 1

_libm = ctypes.CDLL("libm.so.6")
for _n in ("logf", "cosf", "sinf"):
    getattr(_libm, _n).restype = ctypes.c_float
    getattr(_libm, _n).argtypes = [ctypes.c_float]


class TTError(Exception):
    """kind is the Debug form of the reference's TTError; str() is its Display form"""

    def __init__(self, kind, text):
        super().__init__(text)
        self.kind = kind


def fold(terms, start):
    """left-to-right f32 sum along the LAST axis from `start`; Iterator::sum::<f32>() starts at -0.0, `let mut sum = 0.0` at +0.0"""
    terms = np.asarray(terms, dtype=F)
    acc = np.full(terms.shape[:-1], start, dtype=F)
    for j in range(terms.shape[-1]):
        acc = acc + terms[..., j]
    return acc


def dot(a, b):
    return fold(np.asarray(a, dtype=F) * np.asarray(b, dtype=F), NEG0)


def norm(v):
    return np.sqrt(dot(v, v))


def normalize(v):
    """-> (v / n where n > 1e-10, else v as it is; n)"""
    n = norm(v)
    if n > EPS:
        v = v / n
    return v, n


def matmul(a, b):
    """c[i, j] = ((+0.0 + a[i,0] b[0,j]) + a[i,1] b[1,j]) + ..."""
    return fold(a[:, None, :] * b.T[None, :, :], F(0.0))


def frobenius_norm(m):
    return np.sqrt(fold(m.reshape(-1) * m.reshape(-1), NEG0))


class Lcg:
    def __init__(self, seed):
        self.state = (seed + 1) & (2 ** 64 - 1)

    def next_u64(self):
        self.state = (self.state * 6364136223846793005 + 1442695040888963407) & (2 ** 64 - 1)
        return self.state

    def next_f32(self):
        return F(self.next_u64() >> 40) / F(1 << 24)


def gaussian_matrix(rows, cols, seed):
    rng = Lcg(seed)
    total = rows * cols
    data = []
    for _ in range((total + 1) // 2):
        u1 = max(rng.next_f32(), EPS)
        u2 = rng.next_f32()
        r = np.sqrt(F(-2.0) * F(_libm.logf(u1)))
        theta = F(2.0) * F(math.pi) * u2
        data.append(r * F(_libm.cosf(theta)))
        if len(data) < total:
            data.append(r * F(_libm.sinf(theta)))
    return np.asarray(data[:total], dtype=F).reshape(rows, cols)


def qr_orthonormalize(y):
    rows, cols = y.shape
    q_cols = []
    for j in range(cols):
        col = y[:, j].copy()
        for q in q_cols:
            proj = dot(col, q)
            col = col - proj * q
        col, n = normalize(col)
        if n > EPS:
            q_cols.append(col)
    if not q_cols:
        return np.zeros((rows, 0), dtype=F)
    return np.stack(q_cols, axis=1)


def power_start(cols):
    i = np.arange(cols, dtype=np.int64)
    return ((i * 7 + 3) % 13).astype(F) / F(13.0) - F(0.5)


def power_iteration(a, max_iter=20, tol=F(1e-6), trace=None):
    rows, cols = a.shape
    v, _ = normalize(power_start(cols))
    u = np.zeros(rows, dtype=F)
    sigma = F(0.0)
    for it in range(max_iter):
        u, new_sigma = normalize(fold(a * v[None, :], NEG0))
        v, _ = normalize(fold(a.T * u[None, :], NEG0))
        if abs(new_sigma - sigma) < tol * max(sigma, F(1.0)):
            if trace is not None:
                trace.append(it + 1)
            return new_sigma, u, v
        sigma = new_sigma
    if trace is not None:
        trace.append(max_iter)
    return sigma, u, v


def svd_power_iteration(m, max_rank, tolerance, trace=None):
    """-> (u [rows][rank], s [rank], vt [rank][cols]); an empty matrix is EmptyMatrix"""
    if m.size == 0:
        raise TTError("Decompose(EmptyMatrix)", "decomposition error: empty matrix")
    rows, cols = m.shape
    rank = min(max_rank, rows, cols)
    a = m.copy()
    abs_tol = F(tolerance) * frobenius_norm(m)
    us, ss, vs = [], [], []
    for _ in range(rank):
        sigma, u, v = power_iteration(a, trace=trace)
        if sigma < abs_tol:
            break
        ss.append(sigma)
        us.append(u)
        vs.append(v)
        a = a - (sigma * u)[:, None] * v[None, :]
    if not ss:
        return np.zeros((rows, 0), dtype=F), np.zeros(0, dtype=F), np.zeros((0, cols), dtype=F)
    return np.stack(us, axis=1), np.asarray(ss, dtype=F), np.stack(vs, axis=0)


def takes_randomized_path(rows, cols, max_rank):
    rank = min(max_rank, rows, cols)
    return rows > 32 and cols > 32 and rank * 2 < min(rows, cols)


def svd_truncated(m, max_rank, tolerance, trace=None):
    if m.size == 0:
        raise TTError("Decompose(EmptyMatrix)", "decomposition error: empty matrix")
    rows, cols = m.shape
    rank = min(max_rank, rows, cols)
    if not takes_randomized_path(rows, cols, max_rank):
        return svd_power_iteration(m, max_rank, tolerance, trace)
    target = rank + min(5, min(rows, cols) - rank)
    omega = gaussian_matrix(cols, target, rows * 31 + cols)
    basis = qr_orthonormalize(matmul(m, omega))
    empty = (np.zeros((rows, 0), dtype=F), np.zeros(0, dtype=F), np.zeros((0, cols), dtype=F))
    if basis.shape[1] == 0:
        return empty
    projected = matmul(np.ascontiguousarray(basis.T), m)
    us, s, vt = svd_power_iteration(projected, rank, tolerance, trace)
    if s.size == 0:
        return empty
    return matmul(basis, us), s, vt


def rank_bounds(shape, max_rank):
    """the worst-case ranks of a config: r_k <= min(max_rank, left * n_k, remaining)"""
    b = [1]
    for k in range(len(shape) - 1):
        rem = int(np.prod(shape[k + 1:], dtype=np.int64))
        b.append(min(max_rank, b[-1] * shape[k], rem))
    return b + [1]


def max_storage(shape, max_rank):
    b = rank_bounds(shape, max_rank)
    return sum(b[k] * shape[k] * b[k + 1] for k in range(len(shape)))


def tt_decompose(vector, shape, max_rank, tolerance, trace=None):
    """-> (ranks, [core k as f32 [r_k][n_k][r_{k+1}]]); raises TTError as the reference returns Err"""
    vector = np.asarray(vector, dtype=F).reshape(-1)
    shape = [int(x) for x in shape]
    if vector.size == 0:
        raise TTError("EmptyVector", "empty vector")
    product = int(np.prod(shape, dtype=object)) if shape else 1
    if product != vector.size:
        raise TTError(f"ShapeMismatch {{ dim: {vector.size}, shape: {shape}, product: {product} }}",
                      f"dimension {vector.size} cannot be reshaped to {shape} (product: {product})")
    if max_rank < 1:
        raise TTError("InvalidRank", "invalid TT-rank: must be >= 1")
    n = len(shape)
    cores, ranks = [], [1]
    cur, left = vector.copy(), 1
    for k in range(n - 1):
        mode = shape[k]
        rem = int(np.prod(shape[k + 1:], dtype=np.int64))
        rows = left * mode
        m = cur.reshape(rows, cur.size // rows) if rows and cur.size else np.zeros((0, 0), dtype=F)
        u, s, vt = svd_truncated(m, max_rank, tolerance, trace)
        new_rank = min(s.size, max_rank)
        ranks.append(new_rank)
        cores.append(np.ascontiguousarray(u[:, :new_rank]).reshape(left, mode, new_rank))
        cur = (s[:new_rank, None] * vt[:new_rank]).reshape(-1) if new_rank else np.zeros(0, dtype=F)
        assert cur.size == new_rank * rem
        left = new_rank
    ranks.append(1)
    cores.append(cur.reshape(left, shape[-1], 1).copy())
    return ranks, cores


def decompose_batch(vectors, shape, max_rank, tolerance):
    """what nmn_tt_decompose returns: status [n], ranks [n][d + 1] (zeros where the status is not Ok), core_off [n + 1], cores"""
    vectors = np.asarray(vectors, dtype=F)
    d = len(shape)
    status = np.zeros(len(vectors), dtype=np.uint32)
    ranks = np.zeros((len(vectors), d + 1), dtype=np.uint32)
    off = np.zeros(len(vectors) + 1, dtype=np.uint64)
    flats = [np.zeros(0, dtype=F)]
    for q, v in enumerate(vectors):
        try:
            r, cores = tt_decompose(v, shape, max_rank, tolerance)
            ranks[q] = r
            flats += [c.reshape(-1) for c in cores]
            off[q + 1] = off[q] + np.uint64(sum(c.size for c in cores))
        except TTError as e:
            assert e.kind == "Decompose(EmptyMatrix)"
            status[q] = EMPTY_MATRIX
            off[q + 1] = off[q]
    return status, ranks, off, np.concatenate(flats).astype(F)


def tt_reconstruct(shape, ranks, cores):
    """f64 contraction, for the round-trip KAT's relative error only (the bit-exact one is tests/_hnsw_tt_oracle.py)"""
    full = cores[0].astype(np.float64)[0]
    for c in cores[1:]:
        full = np.tensordot(full, c.astype(np.float64), axes=([full.ndim - 1], [0]))
    return full.reshape(-1)


def optimal_shape(dim):
    table = {64: [4, 4, 4], 128: [4, 4, 8], 256: [4, 8, 8], 384: [4, 8, 12], 512: [8, 8, 8], 768: [8, 8, 12], 1024: [8, 8, 16],
             1536: [8, 12, 16], 2048: [8, 16, 16], 3072: [8, 16, 24], 4096: [8, 8, 8, 8], 8192: [8, 8, 8, 16]}
    return table.get(dim) or factorize_balanced(dim)


def factorize_balanced(n):
    if n == 0:
        return []
    if n == 1:
        return [1]
    target_factors = min(max(int(math.ceil(math.log2(n))), 2), 6)
    target_size = int(float(n) ** (1.0 / target_factors))
    factors, remaining = [], n
    for _ in range(target_factors - 1):
        best = 1
        for f in range(max(target_size, 2), 1, -1):
            if remaining % f == 0:
                best = f
                break
        if best == 1:
            for f in range(2, remaining + 1):
                if remaining % f == 0:
                    best = f
                    break
        factors.append(best)
        remaining //= best
        if remaining == 1:
            break
    if remaining > 1:
        factors.append(remaining)
    return sorted(factors)


PRESETS = {"for_dim": (8, 1e-4), "high_compression": (4, 1e-2), "high_accuracy": (16, 1e-6)}


def config_for_dim(dim, preset="for_dim"):
    if dim == 0:
        raise TTError("EmptyVector", "empty vector")
    r, t = PRESETS[preset]
    return optimal_shape(dim), r, F(t)


def rank_one(rng, shape):
    """an exactly representable outer product of small integers"""
    fs = [rng.integers(1, 4, n).astype(np.float64) for n in shape]
    full = fs[0]
    for f in fs[1:]:
        full = np.multiply.outer(full, f)
    return full.reshape(-1).astype(F)


def gpu_cases():
    """(name, shape, max_rank, tolerance, vectors): the list of the GPU test, shared with the CPU test of the host path"""
    rng = np.random.default_rng(20260)
    rnd = lambda n, d: rng.standard_normal((n, d)).astype(F)   # noqa: E731
    sin64 = np.sin(F(0.1) * np.arange(64, dtype=F)).astype(F)
    cases = [("sin_and_random_444", (4, 4, 4), 8, 1e-4, np.vstack([sin64[None], rnd(3, 64)])),
             ("sin_kat_444", (4, 4, 4), 16, 1e-8, sin64[None]),
             ("random_448", (4, 4, 8), 8, 1e-4, rnd(3, 128))]
    v768 = rnd(2, 768)
    for name, (r, t) in PRESETS.items():
        cases.append((f"8x8x12_{name}", (8, 8, 12), r, t, v768))
    cases.append(("randomized_33x34", (33, 34), 4, 1e-4, rnd(2, 1122)))
    cases.append(("randomized_middle_8888", (8, 8, 8, 8), 8, 1e-4, rnd(2, 4096)))
    cases.append(("rank_one_234", (2, 3, 4), 8, 1e-4, np.stack([rank_one(rng, (2, 3, 4)) for _ in range(2)])))
    cases.append(("zero_234", (2, 3, 4), 8, 1e-4, np.zeros((1, 24), dtype=F)))
    cases.append(("zero_34", (3, 4), 8, 1e-4, np.zeros((1, 12), dtype=F)))
    mixed = np.vstack([rnd(8, 64), np.stack([rank_one(rng, (4, 4, 4)) for _ in range(8)])])
    cases.append(("tolerance_0p9_444", (4, 4, 4), 8, 0.9, mixed))
    cases.append(("rank_zero_88", (8, 8), 8, 0.9, rnd(2, 64)))
    base = rnd(1, 128)
    cases.append(("scaled_448", (4, 4, 8), 8, 1e-4, np.vstack([base * F(1e-12), base * F(1e-30), base * F(1e15)])))
    return cases


def big_batch():
    """300 vectors of (4,4,8) mixing random, rank-one, rank-two and zero vectors"""
    rng = np.random.default_rng(20261)
    v = rng.standard_normal((300, 128)).astype(F)
    for q in range(0, 300, 3):
        v[q] = rank_one(rng, (4, 4, 8))
    for q in range(2, 300, 30):
        v[q] = rank_one(rng, (4, 4, 8)) + F(0.5) * rank_one(rng, (4, 4, 8))[::-1]
    v[1::50] = 0.0
    return (4, 4, 8), 8, 1e-4, v
