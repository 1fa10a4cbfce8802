"""CPU restatement of the reference's HNSW index holding TensorTrain nodes beside Dense and Sparse ones — TEST INFRASTRUCTURE ONLY.

Written from the reference's text, independently of the product (neumann_amd/csrc/nmn_hnsw*.hip); paths relative to the reference
root, all in tensor_store/src/hnsw.rs:
  TTVectorCached::new 276-289 (the train and norm = tt_norm(tt)), From<TTVector> 1256-1259, insert_embedding 1913-1927,
  try_insert_embedding 1936-2051 (the insert-time query is embedding.to_dense(), 1985: tt_reconstruct, 620),
  dot_with_dense 793-796 / dot_with_sparse 884-887 (on the reconstruction), magnitude 976 / 1023 (the CACHED norm),
  cosine_distance_dense 1035-1045, cosine_distance_sparse 1069-1079 (`== 0.0` tests), euclidean_distance_dense / _sparse
  1093-1096 / 1116-1120, dot_product_distance_* 1136-1145,
  cosine_distance_tt_with_norm 1196-1221 (a TensorTrain node: tt_dot_product(node, query), 1.0 on Err, `< 1e-10` tests),
  memory_bytes 1230 (4 storage_size()),
  try_cosine_distance T x T 2460-2468, T x D 2469-2480, T x S 2481-2485; try_euclidean_distance 2566-2581;
  try_dot_product_distance 2644-2658.

`HNSWTTNodeIndex` is `_hnsw_mixed_oracle.HNSWMixedIndex` with one more kind per node: the walk, the heaps and the pruning loop are
`_hnsw_oracle.HNSWIndex`'s, only the distance hooks and the bookkeeping change.  `rows[node]` of a TT node is its reconstruction and
`mags[node]` simd::magnitude of that row (what the parent's insert stores: the T x D arm's mag_a); the cached norm sits in `tt`.
"""
import numpy as np

from tests import _hnsw_mixed_oracle as mo
from tests import _hnsw_oracle as ho
from tests import _hnsw_tt_oracle as to
from tests import _tt_similarity_oracle as so

F = np.float32
TINY = F(1e-10)   # the f32 nearest to 1e-10, as the literals in `norm < 1e-10` are


class HNSWTTNodeIndex(mo.HNSWMixedIndex):
    def __init__(self, config=None):
        super().__init__(config)
        self.tt = {}     # node -> (TTVector, cached norm f32)

    def kind(self, node):
        return "tt" if node in self.tt else super().kind(node)

    def magnitude(self, node):
        """EmbeddingStorage::magnitude of a Dense or TensorTrain node (976, 1023)"""
        return self.tt[node][1] if node in self.tt else self.mags[node]

    # ---- the query side: a dense or sparse query (rule 1) ---------------------------------------------------------------------
    def _dense_nodes_query(self, ids, q, qmag):
        """Dense and TensorTrain nodes: the dot on the row (a TT node's reconstruction), magnitude() under Cosine"""
        metric = self.config.distance_metric
        ids = list(ids)
        if self._sq is None or metric == ho.EUCLIDEAN:
            if metric == ho.EUCLIDEAN:
                return ho.euclidean_distance_rows(self.rows[ids], q)
            dot = ho.dot_product_rows(self.rows[ids], q)
        else:
            dot = self._sq.dot_dense_rows(self.rows[ids])
        if metric == ho.DOT_PRODUCT:
            return -dot
        return np.array([mo._cosine(x, self.magnitude(i), qmag) for x, i in zip(dot, ids)], dtype=F)

    def search_sparse_with_ef(self, sq, k, ef):
        """search_sparse_with_ef 2118-2166: the parent's, on a copy of THIS class (its copy is a HNSWMixedIndex)"""
        w = HNSWTTNodeIndex.__new__(HNSWTTNodeIndex)
        w.__dict__.update(self.__dict__)
        w._sq = sq
        w.distance_evals = 0
        res = w.search_with_ef(sq.to_dense(), k, ef)
        self.distance_evals += w.distance_evals
        return res

    # ---- the query side: a TT query (rule 2) ----------------------------------------------------------------------------------
    def tt_node_distance(self, node, query_tt, query_norm):
        """cosine_distance_tt_with_norm on a TensorTrain node, 1196-1209"""
        if query_norm < TINY:
            return F(1.0)
        tt, norm = self.tt[node]
        try:
            dot = so.tt_dot_product(tt, query_tt)        # node first, query second
        except so.TTError:
            return F(1.0)
        if norm < TINY:
            return F(1.0)
        with np.errstate(all="ignore"):
            return F(1.0) - (dot / (norm * query_norm))

    def cosine_distance_tt_with_norm(self, ids, query_tt, q, query_norm):
        ids = [int(i) for i in ids]
        out = np.empty(len(ids), dtype=F)
        rest = [(p, i) for p, i in enumerate(ids) if i not in self.tt]
        if rest:
            out[[p for p, _ in rest]] = to.cosine_distance_tt_with_norm(self, [i for _, i in rest], q, query_norm)
        for p, i in enumerate(ids):
            if i in self.tt:
                out[p] = self.tt_node_distance(i, query_tt, query_norm)
        return out

    def search_tt_with_ef(self, tt, k, ef):
        """search_tt_with_ef 1811-1841 over all node kinds -> [(id, score f32)]"""
        if self.entry_point is None:
            return []
        q = to.tt_reconstruct(tt)
        norm = to.tt_norm(tt)
        w = object.__new__(ho.HNSWIndex)
        w.__dict__.update(self.__dict__)
        w.distance_evals = 0
        w._dist_query = lambda ids, qq, qmag: self.cosine_distance_tt_with_norm(ids, tt, q, norm)
        current = w.entry_point
        for layer in range(w.max_layer, 0, -1):
            current = w.search_layer_greedy(q, norm, current, layer)
        cand = w.search_layer(q, norm, current, max(ef, k), 0)
        return [(nid, F(1.0) - F(d)) for d, nid in cand[:k]]

    # ---- the pruning side (rules 3 and 4) -------------------------------------------------------------------------------------
    def _pair_tt(self, a, b):
        """try_*_distance with a TensorTrain node in the pair"""
        metric = self.config.distance_metric
        ta, tb = a in self.tt, b in self.tt
        t, o = (a, b) if ta else (b, a)
        recon = self.rows[t]
        s = self.sparse.get(o)
        if s is not None:                                            # T x S
            if metric == ho.EUCLIDEAN:
                return ho.euclidean_distance_rows(recon[None, :], s.to_dense())[0]
            if metric == ho.DOT_PRODUCT:
                return -s.dot_dense(recon)
            return s.cosine_distance_dense(recon)
        if metric == ho.EUCLIDEAN:                                   # T x T and T x D: the dense arithmetic on the reconstruction
            return ho.euclidean_distance_rows(recon[None, :], self.rows[o])[0]
        dot = ho.dot_product_rows(recon[None, :], self.rows[o])[0]
        if metric == ho.DOT_PRODUCT:
            return -dot
        if ta and tb:                                                # 2460-2468: the cached norms, `< 1e-10`, no `== 0.0`
            na, nb = self.tt[a][1], self.tt[b][1]
            if na < TINY or nb < TINY:
                return F(1.0)
            with np.errstate(all="ignore"):
                return F(1.0) - (dot / (na * nb))
        return mo._cosine(dot, self.mags[t], self.mags[o])           # 2469-2480: simd::magnitude of both, `== 0.0`

    def _dist_pairs(self, a_id, ids):
        ids = list(ids)
        out = np.empty(len(ids), dtype=F)
        rest = [k for k, i in enumerate(ids) if a_id not in self.tt and i not in self.tt]
        if rest:
            out[rest] = super()._dist_pairs(a_id, [ids[k] for k in rest])
        for k, i in enumerate(ids):
            if a_id in self.tt or i in self.tt:
                out[k] = self._pair_tt(a_id, i)
        return out

    # ---- insertion ------------------------------------------------------------------------------------------------------------
    def insert_embedding_tt(self, tt):
        """insert_embedding(EmbeddingStorage::from(tt)): the kind and the cached norm in place before the walk"""
        node_id = self.n
        self.tt[node_id] = (tt, to.tt_norm(tt))
        try:
            return self._insert_embedding(to.tt_reconstruct(tt), None)   # the query is to_dense(): a dense walk
        except Exception:
            self.tt.pop(node_id, None)
            raise

    def memory_stats(self):
        dim = self.rows.shape[1] if self.rows is not None else 0
        ns, nt = len(self.sparse), len(self.tt)
        return {"total_nodes": self.n, "dense_count": self.n - ns - nt, "sparse_count": ns, "tt_count": nt,
                "embedding_bytes": (self.n - ns - nt) * 4 * dim + sum(s.memory_bytes() for s in self.sparse.values())
                + sum(4 * t.flat().size for t, _ in self.tt.values())}


def answers_tt(idx, tts, k, ef=None):
    return mo.padded([idx.search_tt_with_ef(t, k, idx.config.ef_search if ef is None else ef) for t in tts], k)


def build(items, config=None):
    """items: ("tt", TTVector) | ("dense", row) | ("sparse", SparseVector), inserted in order"""
    idx = HNSWTTNodeIndex(config)
    for kind, x in items:
        if kind == "tt":
            idx.insert_embedding_tt(x)
        elif kind == "sparse":
            idx.insert_sparse(x)
        else:
            idx.insert(np.asarray(x, dtype=F))
    return idx


def lists_differ(a, b):
    """nodes whose neighbour lists differ between two indexes of the same levels"""
    return sum(1 for x, y in zip(a.neighbors, b.neighbors) if x != y)


def answers_differ(a, b):
    """queries whose ids or score bits differ between two padded answers"""
    return int(((a[0] != b[0]) | (a[1].view(np.uint32) != b[1].view(np.uint32))).any(axis=1).sum())


# ---- tests/golden/hnsw_ttnode_small.npz (written by tests/golden/make_golden_hnsw_ttnode.py) -----------------------------------
GOLDEN_SHAPE, GOLDEN_RANKS, GOLDEN_SEED, GOLDEN_N, GOLDEN_NQ = [2, 2, 5], [1, 2, 2, 1], 0x7714, 400, 64


def golden_sets():
    """400 Gaussian trains of shape [2,2,5], ranks [1,2,2,1]; one in eight has every core scaled by 10^-e, e uniform in [3.0, 4.2]:
    the norm scales by 10^-3e, so those norms spread over [4e-13, 1e-9] around 1e-10.  Every second node (the odd ids) is inserted
    as a TT node, the others as Dense(reconstruction).  64 Gaussian dense queries; 64 TT queries, the first 8 of them tiny as well."""
    rng = np.random.default_rng(GOLDEN_SEED)
    trains = []
    for i in range(GOLDEN_N):
        scale = 1.0 if i % 8 != 3 else 10.0 ** -rng.uniform(3.0, 4.2)
        trains.append(to.random_tt(rng, GOLDEN_SHAPE, GOLDEN_RANKS, scale))
    tt_mask = np.arange(GOLDEN_N) % 2 == 1
    dense_q = rng.standard_normal((GOLDEN_NQ, 20)).astype(F)
    tt_q = [to.random_tt(rng, GOLDEN_SHAPE, GOLDEN_RANKS, 10.0 ** -rng.uniform(3.0, 4.2) if j < 8 else 1.0) for j in range(GOLDEN_NQ)]
    return trains, tt_mask, dense_q, tt_q


def golden_index(trains, tt_mask, metric, as_dense=False):
    cfg = ho.HNSWConfig().with_distance_metric(metric)
    return build([("tt", t) if m and not as_dense else ("dense", to.tt_reconstruct(t)) for t, m in zip(trains, tt_mask)], cfg)
