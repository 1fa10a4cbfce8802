"""CPU restatement of the reference's IVF-PQ and IVF-Binary storages — TEST INFRASTRUCTURE ONLY.

The product runs all of this on the GPU (neumann_amd/csrc/nmn_ivf.hip + nmn_ivf_codec.hip: nmn_ivf_build_ex / nmn_ivf_add /
nmn_ivf_search).  Written from the reference's text (paths relative to the reference root):
  tensor_store/src/pq.rs                  PQConfig 40-85, PQCodebook::train 114-169, encode 203-239,
                                          compute_adc_table 268-296, squared_euclidean 331-338,
                                          ADCTable::squared_distance / distance 392-413
  tensor_store/src/binary_quantization.rs BinaryThreshold::compute 27-60, from_dense 70-88, hamming_distance 108-115,
                                          normalized_distance 128-134
  tensor_store/src/ivf.rs                 train 222-274 (residuals 235-249), add 276-316, search_with_nprobe 325-406
  vector_engine/src/lib.rs                estimate_ivf_memory 2821-2851

Centroids, list assignment and the k-means are IVF-Flat's: kmeans_fit / nearest_centroid / sq_dist_rows of
oracle/ivf_oracle.py.  Every sum here is an explicit sequential f32 loop (np.sum is pairwise and would round differently).
"""
import numpy as np

from oracle.ivf_oracle import F, KMeansConfig, default_nprobe, kmeans_fit, nearest_centroid, sq_dist_rows  # noqa: F401

F32_MAX = np.finfo(F).max


# ---- PQ (pq.rs) ---------------------------------------------------------------------------------------------------
class PQConfig:
    def __init__(self, num_subspaces=8, num_centroids=256, kmeans_config=None):
        self.num_subspaces = num_subspaces
        self.num_centroids = num_centroids
        self.kmeans_config = kmeans_config or KMeansConfig()

    @staticmethod
    def high_compression():
        return PQConfig(num_subspaces=4)

    @staticmethod
    def high_recall():
        return PQConfig(num_subspaces=32)


class PQCodebook:
    """centroids [M][K][subdim] f32 (pq.rs:96-110)"""

    def __init__(self, subspace_dim, num_subspaces, num_centroids, centroids, original_dim):
        self.subspace_dim = subspace_dim
        self.num_subspaces = num_subspaces
        self.num_centroids = num_centroids
        self.centroids = np.asarray(centroids, dtype=F).reshape(num_subspaces, num_centroids, subspace_dim) \
            if subspace_dim else np.zeros((num_subspaces, 0, 0), dtype=F)
        self.original_dim = original_dim

    @staticmethod
    def train(vectors, config):
        vectors = np.asarray(vectors, dtype=F)
        if vectors.shape[0] == 0:
            return PQCodebook(0, config.num_subspaces, config.num_centroids, [], 0)
        dim = vectors.shape[1]
        if config.num_subspaces == 0 or dim % config.num_subspaces != 0:
            raise ValueError(f"Vector dimension ({dim}) must be divisible by num_subspaces ({config.num_subspaces})")
        sub = dim // config.num_subspaces
        K = min(config.num_centroids, vectors.shape[0])
        cb = np.zeros((config.num_subspaces, K, sub), dtype=F)
        for m in range(config.num_subspaces):
            cents = kmeans_fit(vectors[:, m * sub:(m + 1) * sub], K, config.kmeans_config)
            cb[m, :len(cents)] = cents  # fewer codewords than asked: zero padding (pq.rs:150-157)
        return PQCodebook(sub, config.num_subspaces, K, cb, dim)

    def encode(self, v):
        v = np.asarray(v, dtype=F)
        if self.subspace_dim == 0 or v.shape[0] != self.original_dim:
            return np.zeros(self.num_subspaces, dtype=np.uint8)
        codes = np.zeros(self.num_subspaces, dtype=np.uint8)
        sub = self.subspace_dim
        for m in range(self.num_subspaces):
            d = sq_dist_rows(self.centroids[m], v[m * sub:(m + 1) * sub]) if self.num_centroids else []
            best, best_idx = F32_MAX, 0
            for k in range(self.num_centroids):
                if d[k] < best:  # `dist < best_dist` from f32::MAX: the first minimum, NaN never wins
                    best, best_idx = d[k], k
            codes[m] = best_idx & 0xFF  # `k as u8`
        return codes

    def encode_rows(self, R):
        """encode for every row of R [n][original_dim] -> u8 [n][M]: vectorised over rows and codewords, each distance a
        sequential f32 sum over the subspace's dimensions as in sq_dist_rows"""
        R = np.asarray(R, dtype=F)
        codes = np.zeros((R.shape[0], self.num_subspaces), dtype=np.uint8)
        if self.subspace_dim == 0 or R.shape[1] != self.original_dim or self.num_centroids == 0:
            return codes
        sub = self.subspace_dim
        for m in range(self.num_subspaces):
            acc = np.full((R.shape[0], self.num_centroids), -0.0, dtype=F)
            for d in range(sub):
                t = self.centroids[m, :, d][None, :] - R[:, m * sub + d][:, None]  # (codeword - v), as sq_dist_rows(cb, v)
                acc = acc + t * t
            best = np.argmin(acc, axis=1)  # NaN-free: the first minimum = the first k with `dist < best_dist` ...
            won = acc[np.arange(R.shape[0]), best] < F32_MAX  # ... unless no distance is below f32::MAX: index 0 stays
            codes[:, m] = (np.where(won, best, 0) & 0xFF).astype(np.uint8)
        return codes

    def decode(self, codes):
        if self.subspace_dim == 0:
            return np.zeros(0, dtype=F)
        return np.concatenate([self.centroids[m, int(c)] if int(c) < self.num_centroids else np.zeros(self.subspace_dim, F)
                               for m, c in enumerate(codes)]).astype(F)

    def compute_adc_table(self, q):
        """[M][K] f32, or an empty table (subspace_dim 0 / wrong length)"""
        q = np.asarray(q, dtype=F)
        if self.subspace_dim == 0 or q.shape[0] != self.original_dim:
            return np.zeros((self.num_subspaces, 0), dtype=F)
        sub = self.subspace_dim
        t = np.zeros((self.num_subspaces, self.num_centroids), dtype=F)
        for m in range(self.num_subspaces):
            if self.num_centroids:
                t[m] = sq_dist_rows(self.centroids[m], q[m * sub:(m + 1) * sub])
        return t


def adc_squared_distance(table, codes):
    if table.size == 0 or len(codes) != table.shape[0]:
        return F32_MAX
    s = F(-0.0)
    for m, c in enumerate(codes):
        s = F(s + table[m, int(c)])
    return s


def adc_distance(table, codes):
    return F(np.sqrt(adc_squared_distance(table, codes)))


def adc_distances(table, codes):
    """adc_distance for every row of codes [n][M] (vectorised over rows, sequential over m)"""
    codes = np.asarray(codes)
    if table.size == 0:
        return np.full(codes.shape[0], np.sqrt(F32_MAX), dtype=F)
    s = np.full(codes.shape[0], -0.0, dtype=F)
    for m in range(codes.shape[1]):
        s = s + table[m, codes[:, m].astype(np.int64)]
    return np.sqrt(s).astype(F)


# ---- Binary (binary_quantization.rs) ------------------------------------------------------------------------------
def threshold(v, method):
    v = np.asarray(v, dtype=F)
    if method == "sign":
        return F(0.0)
    if len(v) == 0:
        return F(0.0)
    if method == "mean":
        s = F(-0.0)
        for x in v:
            s = F(s + x)
        return F(s / F(len(v)))
    if method == "median":
        srt = sorted(v.tolist())  # (NaN-free rows: any sort gives the reference's order up to equal elements)
        mid = len(srt) // 2
        if len(srt) % 2 == 0:
            return F((float(F(srt[mid - 1])) + float(F(srt[mid]))) / 2.0)  # f32::midpoint: through f64 on x86-64
        return F(srt[mid])
    raise ValueError(method)


def from_dense(v, method):
    """-> u64 words, bit i of word i // 64 = v[i] > threshold"""
    v = np.asarray(v, dtype=F)
    t = threshold(v, method)
    words = np.zeros((len(v) + 63) // 64, dtype=np.uint64)
    for i, x in enumerate(v):
        if x > t:
            words[i // 64] |= np.uint64(1) << np.uint64(i % 64)
    return words


def thresholds_rows(V, method):
    """threshold for every row of V [n][dim] (dim >= 1): vectorised over rows, the Mean's sum sequential over the columns"""
    V = np.asarray(V, dtype=F)
    n, dim = V.shape
    if method == "sign":
        return np.zeros(n, dtype=F)
    if method == "mean":
        s = np.full(n, -0.0, dtype=F)
        for j in range(dim):
            s = s + V[:, j]
        return (s / F(dim)).astype(F)
    if method == "median":
        srt = np.sort(V, axis=1)  # (NaN-free rows; -0.0 and +0.0 compare equal, and `v > t` is the same for either)
        mid = dim // 2
        if dim % 2 == 0:
            return ((srt[:, mid - 1].astype(np.float64) + srt[:, mid].astype(np.float64)) / 2.0).astype(F)
        return srt[:, mid].copy()
    raise ValueError(method)


def from_dense_rows(V, method):
    """from_dense for every row of V [n][dim] -> u64 [n][ceil(dim / 64)]"""
    V = np.asarray(V, dtype=F)
    n, dim = V.shape
    W = (dim + 63) // 64
    if dim == 0:
        return np.zeros((n, 0), dtype=np.uint64)
    bits = V > thresholds_rows(V, method)[:, None]
    packed = np.zeros((n, W * 8), dtype=np.uint8)
    packed[:, :(dim + 7) // 8] = np.packbits(bits, axis=1, bitorder="little")
    return np.ascontiguousarray(packed).view("<u8").astype(np.uint64)


def hamming(a, b):
    return int(sum(bin(int(x) ^ int(y)).count("1") for x, y in zip(a, b)))


def normalized_distance(a, b, dim):
    if dim == 0:
        return F(0.0)
    return F(F(hamming(a, b)) / F(dim))


def normalized_distances(qwords, words, dim):
    """normalized_distance(qwords, row, dim) for every row of words [n][W]"""
    words = np.asarray(words, dtype=np.uint64)
    if dim == 0:
        return np.zeros(words.shape[0], dtype=F)
    x = np.ascontiguousarray(words ^ np.asarray(qwords, dtype=np.uint64)[None, :])
    h = np.unpackbits(x.view(np.uint8), axis=1).sum(axis=1, dtype=np.int64)
    return (h.astype(F) / F(dim)).astype(F)  # hamming <= dim < 2^24: `as f32` is exact


def assign_rows(V, centroids):
    """nearest_centroid(v, centroids) for every row of V (NaN-free rows: np.argmin is the first minimum)"""
    V = np.asarray(V, dtype=F)
    D = np.stack([sq_dist_rows(V, c) for c in np.asarray(centroids, dtype=F)], axis=1)  # (v - c)^2 = (c - v)^2 bit for bit
    if np.isnan(D).any():
        return np.array([nearest_centroid(v, centroids) for v in V], dtype=np.int64)
    return np.argmin(D, axis=1)


# ---- IVFIndex with PQ / Binary storage (ivf.rs) ------------------------------------------------------------------
class IVFCoded:
    """IVFIndex with IVFStorage::PQ(pq_config) (storage="pq") or IVFStorage::Binary(threshold) (storage="binary")."""

    def __init__(self, num_clusters, storage, pq_config=None, threshold="sign", nprobe=None, kmeans=None):
        self.num_clusters = num_clusters
        self.storage = storage
        self.pq_config = pq_config or PQConfig()
        self.threshold = threshold
        self.nprobe = default_nprobe(num_clusters) if nprobe is None else nprobe
        self.kmeans = kmeans or KMeansConfig()
        self.centroids = None
        self.codebook = None
        self.lists = []
        self.codes = []   # id -> codes (PQ: u8 [M]; Binary: u64 words)
        self.assign = []

    def train(self, vectors):
        vectors = np.asarray(vectors, dtype=F)
        if vectors.shape[0] == 0:
            return
        self.centroids = kmeans_fit(vectors, min(self.num_clusters, vectors.shape[0]), self.kmeans)
        if self.storage == "pq":
            res = np.stack([v - self.centroids[nearest_centroid(v, self.centroids)] for v in vectors]).astype(F)
            self.codebook = PQCodebook.train(res, self.pq_config)
        self.lists = [[] for _ in range(len(self.centroids))]
        self.codes, self.assign = [], []

    def set_trained(self, centroids, codebook=None):
        """the state train() leaves, from given centroids (and codebook)"""
        self.centroids = np.asarray(centroids, dtype=F)
        self.codebook = codebook
        self.lists = [[] for _ in range(len(self.centroids))]
        self.codes, self.assign = [], []

    def add(self, v):
        v = np.asarray(v, dtype=F)
        c = nearest_centroid(v, self.centroids)
        vid = len(self.codes)
        if self.storage == "pq":
            self.codes.append(self.codebook.encode((v - self.centroids[c]).astype(F)))
        else:
            self.codes.append(from_dense(v, self.threshold))
        self.assign.append(c)
        self.lists[c].append(vid)
        return vid

    def add_rows(self, V):
        """add(v) for every row of V through the batch helpers: codes, assign and lists end as repeated add leaves them.
        Returns the clusters chosen."""
        V = np.asarray(V, dtype=F)
        a = assign_rows(V, self.centroids)
        if self.storage == "pq":
            new = self.codebook.encode_rows((V - self.centroids[a]).astype(F))
        else:
            new = from_dense_rows(V, self.threshold)
        for c, row in zip(a.tolist(), new):
            self.lists[c].append(len(self.codes))
            self.codes.append(row.copy())
            self.assign.append(c)
        return a

    def cluster_sizes(self):
        return [len(lst) for lst in self.lists]

    def search(self, q, k, nprobe=None):
        if self.centroids is None or len(self.centroids) == 0 or k == 0:
            return [], np.zeros(0, dtype=F)
        q = np.asarray(q, dtype=F)
        nprobe = self.nprobe if nprobe is None else nprobe
        cd = sq_dist_rows(self.centroids, q)
        order = sorted(range(len(cd)), key=lambda i: float(cd[i]))
        qbits = from_dense(q, self.threshold) if self.storage == "binary" else None
        cand_ids, cand_d = [], []
        for c in order[:min(nprobe, len(order))]:
            ids = self.lists[c]
            if not ids:
                continue
            if self.storage == "pq":
                table = self.codebook.compute_adc_table((q - self.centroids[c]).astype(F))
                d = adc_distances(table, np.stack([self.codes[i] for i in ids]))
            else:
                d = normalized_distances(qbits, np.stack([self.codes[i] for i in ids]), len(q))
            cand_ids.extend(ids)
            cand_d.extend(d.tolist())
        order2 = sorted(range(len(cand_d)), key=lambda i: cand_d[i])  # stable: probe order, then list order
        order2 = order2[:k]
        return [cand_ids[i] for i in order2], np.array([cand_d[i] for i in order2], dtype=F)


def estimate_ivf_memory(count, dim, num_clusters, storage, num_subspaces=8):
    """estimate_ivf_memory (lib.rs:2821-2851)"""
    if count == 0:
        return 0
    vec = {"flat": count * dim * 4, "pq": count * num_subspaces, "binary": count * ((dim + 63) // 64) * 8}[storage]
    return num_clusters * dim * 4 + vec + count * 8
