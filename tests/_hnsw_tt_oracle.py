"""CPU restatement of the reference's tensor-train queries of the HNSW index — TEST INFRASTRUCTURE ONLY.

Written from the reference's text, independently of the product (neumann_amd/csrc/nmn_tt.hip, nmn_hnsw.hip); paths relative to the
reference root:
  tensor_compress/src/tensor_train.rs  TTCore::get 240-243 (core k is r_k x n_k x r_{k+1}, element (i, j, r) at (i n_k + j) r_{k+1} + r),
                                       TTVector 267-281, tt_reconstruct 401-436, tt_norm 440-474
  tensor_store/src/hnsw.rs             dot_with_tt 919-948 (the query reconstructed; simd::dot_product on a Dense node, dot_dense of
                                       a Sparse and of a Quantized one), magnitude 950-985, cosine_distance_tt_with_norm 1196-1221,
                                       insert_tt_vector 1755-1759, search_tt_with_ef 1811-1841, search_layer_tt_native 1845-1903,
                                       search_layer_greedy_tt 2238-2272

tt_reconstruct is restated ELEMENT BY ELEMENT as the reference runs it (every element walks all the cores from left = [1.0]; numpy
carries all elements side by side, each keeping its own chain) — not level by level as the kernel shares prefixes.  tt_norm keeps
one chain per (a, b) over k, then i, then j, numpy carrying the (a, b) side by side.  Every operation is one numpy float32 operation:
rounded once, never fused.

search_layer_tt_native and search_layer_greedy_tt are search_layer and search_layer_greedy line by line with the distance replaced
(compared: the visited set, both heaps, the break test, should_add, the trim loop and the final stable sort are the same text), so
the walk is `_hnsw_oracle.HNSWIndex`'s with `_dist_query` swapped — on a dense, a mixed (`_hnsw_mixed_oracle`) or a quantized
(`_hnsw_q8_oracle`) index.  The score is 1.0 - distance whatever the index's metric.
"""
import numpy as np

from tests import _hnsw_mixed_oracle as mo
from tests import _hnsw_oracle as ho
from tests import _hnsw_q8_oracle as qo

F = np.float32
TINY = F(1e-10)   # the f32 nearest to 1e-10, as the literal in `query_norm < 1e-10` is


class TTVector:
    """shape [n_1 .. n_d], ranks [1, r_1 .. r_{d-1}, 1], cores: d arrays [r_{k}, n_k, r_{k+1}] f32"""

    def __init__(self, shape, ranks, cores):
        self.shape = [int(x) for x in shape]
        self.ranks = [int(x) for x in ranks]
        assert len(self.ranks) == len(self.shape) + 1 and self.ranks[0] == 1 and self.ranks[-1] == 1
        self.cores = [np.ascontiguousarray(c, dtype=F).reshape(self.ranks[k], self.shape[k], self.ranks[k + 1])
                      for k, c in enumerate(cores)]

    @property
    def dim(self):
        return int(np.prod(self.shape, dtype=np.int64))

    def flat(self):
        return np.concatenate([c.reshape(-1) for c in self.cores]) if self.cores else np.zeros(0, dtype=F)


def random_tt(rng, shape, ranks, scale=1.0):
    return TTVector(shape, ranks, [(rng.standard_normal((ranks[k], shape[k], ranks[k + 1])) * scale).astype(F)
                                   for k in range(len(shape))])


def pack(tts):
    """-> (shape u32 [d], ranks u32 [nq][d + 1], core_off u64 [nq + 1], cores f32): the C entries' arguments"""
    shape = np.asarray(tts[0].shape, dtype=np.uint32)
    for t in tts:
        assert t.shape == tts[0].shape
    ranks = np.asarray([t.ranks for t in tts], dtype=np.uint32)
    flats = [t.flat() for t in tts]
    off = np.zeros(len(tts) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([f.size for f in flats])
    return shape, ranks, off, (np.concatenate(flats) if flats else np.zeros(0, dtype=F)).astype(F)


def tt_reconstruct(tt):
    total = tt.dim
    flat = np.arange(total, dtype=np.int64)
    multi = []
    remaining = flat
    for n in reversed(tt.shape):           # multi_idx[k] = remaining % shape[k], from the last mode
        multi.append(remaining % n)
        remaining = remaining // n
    multi.reverse()
    left = np.ones((total, 1), dtype=F)   # left_vec = [1.0] for every element
    with np.errstate(all="ignore"):
        for k, core in enumerate(tt.cores):
            r1, _, r2 = core.shape
            new = np.zeros((total, r2), dtype=F)
            for r in range(r2):
                acc = np.zeros(total, dtype=F)
                for l in range(r1):
                    acc = acc + left[:, l] * core[l, multi[k], r]
                new[:, r] = acc
            left = new
    return left[:, 0].copy()


def tt_norm(tt):
    gram = np.ones(1, dtype=F)
    with np.errstate(all="ignore"):
        for core in tt.cores:
            r1, n, r2 = core.shape
            s = np.zeros((r2, r2), dtype=F)
            for k in range(n):
                for i in range(r1):
                    for j in range(r1):
                        g = gram[0] if r1 == 1 else gram[i * r1 + j]
                        s = s + (g * core[i, k, :])[:, None] * core[j, k, :][None, :]
            gram = s.reshape(-1)
        return np.sqrt(gram[0])


def cosine_distance_tt_with_norm(idx, ids, q, query_norm):
    """the distance of every node of `ids` to the train whose reconstruction is q — Dense, Sparse and Quantized nodes"""
    ids = [int(i) for i in ids]
    out = np.empty(len(ids), dtype=F)
    if query_norm < TINY:
        out[:] = F(1.0)
        return out
    with np.errstate(all="ignore"):
        if isinstance(idx, qo.HNSWQ8Index):
            a = np.asarray(ids, dtype=np.int64)
            dot = qo.dot_dense(idx.codes[a], idx.scale[a], idx.min_val[a], q)
            mag = idx.mags[a]
            out[:] = F(1.0) - (dot / (mag * query_norm))
            out[mag == 0] = F(1.0)
            return out
        sparse = getattr(idx, "sparse", {})
        dense = [(p, i) for p, i in enumerate(ids) if i not in sparse]
        if dense:
            a = np.asarray([i for _, i in dense], dtype=np.int64)
            dot = ho.dot_product_rows(idx.rows[a], q)
            mag = idx.mags[a]
            d = F(1.0) - (dot / (mag * query_norm))
            d[mag == 0] = F(1.0)
            out[[p for p, _ in dense]] = d
        for p, i in enumerate(ids):
            if i in sparse:
                s = sparse[i]
                mag = F(s.magnitude())
                out[p] = F(1.0) if mag == 0 else F(1.0) - (F(s.dot_dense(q)) / (mag * query_norm))
    return out


def search_tt_with_ef(idx, tt, k, ef):
    """-> [(id, score f32)]"""
    if idx.entry_point is None:
        return []
    q = tt_reconstruct(tt)
    norm = tt_norm(tt)
    w = object.__new__(ho.HNSWIndex)
    w.__dict__.update(idx.__dict__)
    w.distance_evals = 0
    w._dist_query = lambda ids, qq, qmag: cosine_distance_tt_with_norm(idx, ids, q, norm)
    current = w.entry_point
    for layer in range(w.max_layer, 0, -1):
        current = w.search_layer_greedy(q, norm, current, layer)
    cand = w.search_layer(q, norm, current, max(ef, k), 0)
    return [(nid, F(1.0) - F(d)) for d, nid in cand[:k]]


def answers_tt(idx, tts, k, ef=None):
    return mo.padded([search_tt_with_ef(idx, t, k, idx.config.ef_search if ef is None else ef) for t in tts], k)


def insert_tt_vector(idx, tt):
    return idx.insert(tt_reconstruct(tt))


# ---- tests/golden/hnsw_tt_small.npz (written by tests/golden/make_golden_hnsw_tt.py) ----------------------------------------------
GOLDEN_SHAPE, GOLDEN_RANKS, GOLDEN_SEED = [2, 2, 5], [1, 2, 2, 1], 0x77


def golden_trains(nq=64):
    """64 trains of shape [2,2,5] (the 20 dimensions of _hnsw_oracle.golden_corpus), ranks [1,2,2,1], Gaussian cores"""
    rng = np.random.default_rng(GOLDEN_SEED)
    return [random_tt(rng, GOLDEN_SHAPE, GOLDEN_RANKS) for _ in range(nq)]
