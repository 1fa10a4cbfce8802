"""CPU restatement of the reference's delta vectors — TEST INFRASTRUCTURE ONLY.

Written from the reference's text, independently of the product (neumann_amd/csrc/nmn_delta.hip); lines of
tensor_store/src/delta_vector.rs:
  DeltaVector        try_from_dense_with_reference 113-147, from_dense_with_reference_and_magnitude 151-161, try_from_parts 185-205,
                     to_dense 209-217, magnitude 260-267, memory_bytes 276-280, dot_dense_with_precomputed 296-305, dot_dense 309-312,
                     dot_same_archetype 321-349, sparse_delta_dot 352-370, cosine_similarity_dense 374-388, compression_ratio 410-416
  ArchetypeRegistry  register 442-452, find_best_archetype 480-513, encode 517-526, decode 530-533, dot_delta_dense 537-540,
                     dot_deltas_same_archetype 544-552, discover_archetypes 566-592, encode_batch 598-607, analyze_coverage 614-643

Every operation is one numpy float32 operation: rounded once, never fused.  An iterator's `.sum::<f32>()` folds from -0.0, the
explicit accumulators (`let mut result = 0.0`) from +0.0.  Chains the reference computes independently (one per row, one per
archetype) are carried side by side in numpy arrays; no chain is ever split or reordered.
"""
import numpy as np

from oracle import ivf_oracle as io

F = np.float32
MAX_DIMENSION = 65535
# size_of::<DeltaVector>() on a 64-bit target: archetype_id usize 8 + dimension usize 8 + positions Vec<u16> 24 + deltas Vec<f32> 24
# + cached_magnitude Option<f32> 8 (a 4-byte tag and the f32; f32 has no niche) = 72, already a multiple of the alignment 8
SIZE_OF_DELTA_VECTOR = 72


def dimension_exceeded(dimension):
    return f"dimension {dimension} exceeds maximum {MAX_DIMENSION} (u16::MAX)"


class DeltaVectorError(Exception):
    pass


def bits_of(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


def sum_sq_rows(X):
    """`.map(|x| x * x).sum::<f32>()` of every row"""
    X = np.asarray(X, dtype=F)
    acc = np.full(X.shape[0], -0.0, dtype=F)
    with np.errstate(all="ignore"):
        for j in range(X.shape[1]):
            acc = acc + X[:, j] * X[:, j]
    return acc


def dot_rows(A, v):
    """`a.iter().zip(v).map(|(a, v)| a * v).sum::<f32>()` of every row of A with v"""
    A, v = np.asarray(A, dtype=F), np.asarray(v, dtype=F)
    acc = np.full(A.shape[0], -0.0, dtype=F)
    with np.errstate(all="ignore"):
        for j in range(A.shape[1]):
            acc = acc + A[:, j] * v[j]
    return acc


def dot_all(A, X):
    """dot_rows(A, x) for every row x of X -> f32 [len(X)][len(A)]"""
    A, X = np.asarray(A, dtype=F), np.asarray(X, dtype=F)
    acc = np.full((X.shape[0], A.shape[0]), -0.0, dtype=F)
    with np.errstate(all="ignore"):
        for j in range(A.shape[1]):
            acc = acc + A[None, :, j] * X[:, j, None]
    return acc


class DeltaVector:
    def __init__(self, archetype_id, dimension, positions, deltas, cached_magnitude=None):
        if dimension > MAX_DIMENSION:
            raise DeltaVectorError(dimension_exceeded(dimension))
        self.archetype_id = int(archetype_id)
        self.dimension = int(dimension)
        self.positions = np.asarray(positions, dtype=np.uint16).reshape(-1)
        self.deltas = np.asarray(deltas, dtype=F).reshape(-1)
        self.cached_magnitude = None if cached_magnitude is None else F(cached_magnitude)

    @classmethod
    def from_dense_with_reference(cls, dense, archetype, archetype_id, threshold):
        dense, archetype = np.asarray(dense, dtype=F), np.asarray(archetype, dtype=F)
        if dense.shape[0] > MAX_DIMENSION:
            raise DeltaVectorError(dimension_exceeded(dense.shape[0]))
        with np.errstate(all="ignore"):
            delta = dense - archetype
            keep = np.abs(delta) > F(threshold)          # a NaN on either side compares false
        return cls(archetype_id, dense.shape[0], np.nonzero(keep)[0], delta[keep])

    @classmethod
    def from_dense_with_reference_and_magnitude(cls, dense, archetype, archetype_id, threshold):
        with np.errstate(all="ignore"):
            magnitude = np.sqrt(sum_sq_rows(np.asarray(dense, dtype=F)[None, :])[0])
        d = cls.from_dense_with_reference(dense, archetype, archetype_id, threshold)
        d.cached_magnitude = magnitude
        return d

    def nnz(self):
        return int(self.positions.shape[0])

    def to_dense(self, archetype):
        result = np.array(archetype, dtype=F, copy=True)
        with np.errstate(all="ignore"):
            for pos, delta in zip(self.positions, self.deltas):
                result[pos] = result[pos] + delta
        return result

    def magnitude(self, archetype):
        if self.cached_magnitude is not None:
            return self.cached_magnitude
        with np.errstate(all="ignore"):
            return np.sqrt(sum_sq_rows(self.to_dense(archetype)[None, :])[0])

    def memory_bytes(self):
        return SIZE_OF_DELTA_VECTOR + self.nnz() * 2 + self.nnz() * 4

    def compression_ratio(self):
        dense_bytes = self.dimension * 4
        if dense_bytes == 0:
            return F(1.0)
        return F(F(dense_bytes) / F(self.memory_bytes()))

    def dot_dense_with_precomputed(self, query, archetype_dot_query):
        query = np.asarray(query, dtype=F)
        delta_dot = F(-0.0)
        with np.errstate(all="ignore"):
            for pos, delta in zip(self.positions, self.deltas):
                delta_dot = F(delta_dot + F(delta * query[pos]))
            return F(F(archetype_dot_query) + delta_dot)

    def dot_dense(self, query, archetype):
        return self.dot_dense_with_precomputed(query, dot_rows(np.asarray(archetype, dtype=F)[None, :], query)[0])

    def sparse_delta_dot(self, other):
        result, i, j = F(0.0), 0, 0
        with np.errstate(all="ignore"):
            while i < self.nnz() and j < other.nnz():
                a, b = int(self.positions[i]), int(other.positions[j])
                if a < b:
                    i += 1
                elif a > b:
                    j += 1
                else:
                    result = F(result + F(self.deltas[i] * other.deltas[j]))
                    i += 1
                    j += 1
        return result

    def dot_same_archetype(self, other, archetype, archetype_magnitude_sq):
        archetype = np.asarray(archetype, dtype=F)
        with np.errstate(all="ignore"):
            r_dot_delta_b = F(-0.0)
            for pos, delta in zip(other.positions, other.deltas):
                r_dot_delta_b = F(r_dot_delta_b + F(archetype[pos] * delta))
            delta_a_dot_r = F(-0.0)
            for pos, delta in zip(self.positions, self.deltas):
                delta_a_dot_r = F(delta_a_dot_r + F(delta * archetype[pos]))
            s = F(F(archetype_magnitude_sq) + r_dot_delta_b)
            s = F(s + delta_a_dot_r)
            return F(s + self.sparse_delta_dot(other))

    def cosine_similarity_dense(self, query, archetype, query_magnitude):
        dot = self.dot_dense(query, archetype)
        self_magnitude = self.magnitude(archetype)
        if self_magnitude == 0.0 or query_magnitude == 0.0:
            return F(0.0)
        with np.errstate(all="ignore"):
            return F(dot / F(self_magnitude * F(query_magnitude)))


class CoverageStats:
    def __init__(self, avg_similarity=0.0, avg_compression_ratio=0.0, avg_delta_nnz=0.0, archetype_usage=()):
        self.avg_similarity, self.avg_compression_ratio, self.avg_delta_nnz = F(avg_similarity), F(avg_compression_ratio), F(avg_delta_nnz)
        self.archetype_usage = list(archetype_usage)


class ArchetypeRegistry:
    def __init__(self, max_archetypes):
        self.archetypes, self.magnitude_sq_, self.max_archetypes = [], [], int(max_archetypes)

    def __len__(self):
        return len(self.archetypes)

    def register(self, archetype):
        if len(self.archetypes) >= self.max_archetypes:
            return None
        archetype = np.array(archetype, dtype=F, copy=True)
        self.magnitude_sq_.append(sum_sq_rows(archetype[None, :])[0])
        self.archetypes.append(archetype)
        return len(self.archetypes) - 1

    def get(self, i):
        return self.archetypes[i] if 0 <= i < len(self.archetypes) else None

    def magnitude_sq(self, i):
        return self.magnitude_sq_[i] if 0 <= i < len(self.archetypes) else None

    def find_best_many(self, vectors):
        """find_best_archetype of every row -> (ids int64 [n], sims f32 [n]); None on an empty registry"""
        if not self.archetypes:
            return None
        X = np.asarray(vectors, dtype=F)
        A = np.stack(self.archetypes)
        with np.errstate(all="ignore"):
            query_mag = np.sqrt(sum_sq_rows(X))
            dots = dot_all(A, X)                                             # [n][K]
            arch_mag = np.sqrt(np.asarray(self.magnitude_sq_, dtype=F))
            best_id = np.zeros(X.shape[0], dtype=np.int64)
            best_sim = np.full(X.shape[0], -np.inf, dtype=F)
            for i in range(len(self.archetypes)):                            # in id order, under the strict `>`
                sim = np.zeros(X.shape[0], dtype=F) if arch_mag[i] == 0.0 else dots[:, i] / (arch_mag[i] * query_mag)
                better = sim > best_sim
                best_sim = np.where(better, sim, best_sim)
                best_id = np.where(better, i, best_id)
        zero = query_mag == 0.0                                              # `return Some((0, 0.0))` before the loop
        return np.where(zero, 0, best_id), np.where(zero, F(0.0), best_sim).astype(F)

    def find_best_archetype(self, vector):
        r = self.find_best_many(np.asarray(vector, dtype=F)[None, :])
        return None if r is None else (int(r[0][0]), F(r[1][0]))

    def encode(self, vector, threshold, with_magnitude=False):
        best = self.find_best_archetype(vector)
        if best is None:
            return None
        make = DeltaVector.from_dense_with_reference_and_magnitude if with_magnitude else DeltaVector.from_dense_with_reference
        return make(vector, self.archetypes[best[0]], best[0], threshold)

    def decode(self, delta):
        a = self.get(delta.archetype_id)
        return None if a is None else delta.to_dense(a)

    def dot_delta_dense(self, delta, query):
        a = self.get(delta.archetype_id)
        return None if a is None else delta.dot_dense(query, a)

    def dot_deltas_same_archetype(self, a, b):
        if a.archetype_id != b.archetype_id:
            return None
        arch = self.get(a.archetype_id)
        return None if arch is None else a.dot_same_archetype(b, arch, self.magnitude_sq_[a.archetype_id])

    def discover_archetypes(self, vectors, k, config):
        vectors = np.asarray(vectors, dtype=F)
        if vectors.shape[0] == 0:
            return 0
        k = min(k, vectors.shape[0], self.max_archetypes - len(self))
        if k == 0:
            return 0
        added = 0
        for centroid in io.kmeans_fit(vectors, k, config):
            if self.register(centroid) is not None:
                added += 1
        return added

    def encode_batch(self, vectors, threshold, with_magnitude=False):
        out = []
        for v in np.asarray(vectors, dtype=F):
            d = self.encode(v, threshold, with_magnitude)
            if d is not None:
                out.append((d, d.compression_ratio()))
        return out

    def analyze_coverage(self, vectors, threshold):
        vectors = np.asarray(vectors, dtype=F)
        if vectors.shape[0] == 0 or not self.archetypes:
            return CoverageStats()
        total_similarity, total_compression, total_delta_nnz = F(0.0), F(0.0), 0
        usage = [0] * len(self)
        ids, sims = self.find_best_many(vectors)
        with np.errstate(all="ignore"):
            for v, arch_id, sim in zip(vectors, ids, sims):
                total_similarity = F(total_similarity + sim)
                usage[arch_id] += 1
                delta = self.encode(v, threshold)
                total_compression = F(total_compression + delta.compression_ratio())
                total_delta_nnz += delta.nnz()
            n = F(vectors.shape[0])
            return CoverageStats(F(total_similarity / n), F(total_compression / n), F(F(total_delta_nnz) / n), usage)


# ---- whole sets, in the layout the library's DeltaSet copies out ----------------------------------------------------------------

def pack(deltas):
    """-> dict(archetype_ids u64 [n], indptr u64 [n + 1], positions u16, deltas f32, cached_magnitudes f32 [n], has_cached bool [n])"""
    n = len(deltas)
    ptr = np.zeros(n + 1, dtype=np.uint64)
    for i, d in enumerate(deltas):
        ptr[i + 1] = ptr[i] + np.uint64(d.nnz())
    return dict(archetype_ids=np.asarray([d.archetype_id for d in deltas], dtype=np.uint64), indptr=ptr,
                positions=np.concatenate([d.positions for d in deltas] + [np.zeros(0, dtype=np.uint16)]).astype(np.uint16),
                deltas=np.concatenate([d.deltas for d in deltas] + [np.zeros(0, dtype=F)]).astype(F),
                cached_magnitudes=np.asarray([F(0.0) if d.cached_magnitude is None else d.cached_magnitude for d in deltas], dtype=F),
                has_cached=np.asarray([d.cached_magnitude is not None for d in deltas], dtype=bool))


def unpack(dim, archetype_ids, indptr, positions, deltas, cached_magnitudes=None, has_cached=None):
    out = []
    for i in range(len(archetype_ids)):
        b, e = int(indptr[i]), int(indptr[i + 1])
        cm = None
        if cached_magnitudes is not None and (has_cached is None or has_cached[i]):
            cm = cached_magnitudes[i]
        out.append(DeltaVector(int(archetype_ids[i]), dim, positions[b:e], deltas[b:e], cm))
    return out


def decode_all(reg, deltas):
    return np.stack([reg.decode(d) for d in deltas]) if deltas else np.zeros((0, 0), dtype=F)


def magnitudes(reg, deltas):
    return np.asarray([d.magnitude(reg.get(d.archetype_id)) for d in deltas], dtype=F)


def dot_dense_all(reg, deltas, queries):
    """-> f32 [nq][n]; the archetype's dot is computed once per (query, archetype): the same chain for every row that shares it"""
    queries = np.asarray(queries, dtype=F)
    arch = dot_all(np.stack(reg.archetypes), queries)
    return np.asarray([[d.dot_dense_with_precomputed(q, arch[qi, d.archetype_id]) for d in deltas] for qi, q in enumerate(queries)],
                      dtype=F).reshape(len(queries), len(deltas))


def cosine_dense_all(reg, deltas, queries):
    queries = np.asarray(queries, dtype=F)
    dots = dot_dense_all(reg, deltas, queries)
    mags = magnitudes(reg, deltas)
    with np.errstate(all="ignore"):
        qmag = np.sqrt(sum_sq_rows(queries))
        out = dots / (mags[None, :] * qmag[:, None])
    out[:, mags == 0.0] = F(0.0)
    out[qmag == 0.0, :] = F(0.0)
    return out.astype(F)


def pairs_all(reg, sa, sb, pairs):
    """-> (f32 [n_pairs], ok bool [n_pairs])"""
    out, ok = np.zeros(len(pairs), dtype=F), np.zeros(len(pairs), dtype=bool)
    for i, (ra, rb) in enumerate(pairs):
        v = reg.dot_deltas_same_archetype(sa[int(ra)], sb[int(rb)])
        ok[i] = v is not None
        if v is not None:
            out[i] = v
    return out, ok
