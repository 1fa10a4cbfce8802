"""CPU restatement of the reference's HNSW index whose every node is EmbeddingStorage::Binary — TEST INFRASTRUCTURE ONLY.

Written from the reference's text, independently of the product (neumann_amd/csrc/nmn_hnsw.hip); paths relative to the
reference root:
  tensor_store/src/binary_quantization.rs   BinaryThreshold::compute 41-65, BinaryVector::from_dense 83-99 (both restated in
      tests/_ivf_codec_oracle.py: threshold / from_dense / hamming), hamming_distance 123-129, similarity 137-142
      (`1.0 - (hamming as f32 / dimension as f32)`), to_dense 157-166 (+1.0 for a set bit, -1.0 otherwise — the doc comment says
      "0.0 or 1.0", the code is what counts), memory_bytes 174-179 (8 bytes per word);
  tensor_store/src/hnsw.rs   EmbeddingStorage::Binary 579; dot_dense's arm 801-805 (simd::dot_product(to_dense(), query));
      magnitude's arm 981-984 (`(dimension as f32).sqrt()`, never 0, NOT simd::magnitude of the row); cosine_distance_dense
      1035-1045 (1.0 when the query's magnitude is 0.0); euclidean_distance_dense's arm 1098-1101
      (simd::euclidean_distance(to_dense(), query)); dot_product_distance_dense 1136-1138; try_insert_embedding's query
      `nodes[node_id].embedding.to_dense()` 1985; the (Binary, Binary) arms of try_cosine / euclidean / dot_product_distance:
      `1.0 - ba.similarity(bb)` 2516-2518, simd::euclidean_distance / -simd::dot_product on both to_dense() rows 2605-2609,
      2680-2684.

So the index is the dense oracle over the +-1 rows with two changes.  The QUERY side (`_dist_query`: search_layer* at search and
at insert time) is the dense arithmetic on the +-1 row with sqrt(dim) in place of the row's magnitude — about 2h/d under Cosine
for two +-1 rows h bits apart.  The PRUNING side (`_dist_pairs`) under Cosine is the Hamming formula on the words, about h/d, with
roundings of its own; under Euclidean and DotProduct it is the dense oracle's as it stands.
"""
import numpy as np

from tests import _hnsw_oracle as ho
from tests import _ivf_codec_oracle as co

F = np.float32


def to_dense(words, dim):
    """BinaryVector::to_dense: +1.0 where bit i of word i // 64 is set, -1.0 otherwise"""
    w = np.ascontiguousarray(np.asarray(words, dtype=np.uint64))
    bits = np.unpackbits(w.view(np.uint8), bitorder="little")[:dim]
    return np.where(bits == 1, F(1.0), F(-1.0)).astype(F)


def mag_self(dim):
    """(dimension as f32).sqrt()"""
    return np.sqrt(F(dim))


def similarity(a, b, dim):
    """BinaryVector::similarity (dimension > 0)"""
    return F(F(1.0) - F(F(co.hamming(a, b)) / F(dim)))


def pruning_cosine(a, b, dim):
    """the (Binary, Binary) arm of try_cosine_distance: 1.0 - ba.similarity(bb)"""
    return F(F(1.0) - similarity(a, b, dim))


class HNSWBinIndex(ho.HNSWIndex):
    def __init__(self, config=None, threshold="sign"):
        super().__init__(config)
        self.threshold = threshold
        self.words = None          # [capacity][ceil(dim / 64)] u64
        self.dim = None

    # insert_embedding(EmbeddingStorage::Binary(BinaryVector::from_dense(v, threshold))): the node's own query is to_dense()
    def insert(self, vector):
        v = np.asarray(vector, dtype=F)
        w = co.from_dense(v, self.threshold)
        node_id = self.n
        if self.words is None:
            self.dim = v.size
            self.words = np.zeros((64, w.size), dtype=np.uint64)
        if node_id == self.words.shape[0]:
            self.words = np.concatenate([self.words, np.zeros_like(self.words)])
        self.words[node_id] = w
        return super().insert(to_dense(w, v.size))

    # EmbeddingStorage::distance_dense(Binary rows `ids`, query)
    def _dist_query(self, ids, q, qmag):
        metric = self.config.distance_metric
        ids = np.asarray(ids, dtype=np.int64)
        A = self.rows[ids]                                   # to_dense() of every row
        self.distance_evals += len(ids)
        if metric == ho.EUCLIDEAN:
            return ho.euclidean_distance_rows(A, q)          # (a - b) with a = the row
        dot = ho.dot_product_rows(A, q)
        if metric == ho.DOT_PRODUCT:
            return -dot
        if qmag == 0:
            return np.ones(len(ids), dtype=F)
        return (F(1.0) - (dot / (mag_self(self.dim) * F(qmag)))).astype(F)

    # the (Binary, Binary) arms of try_*_distance
    def _dist_pairs(self, a_id, ids):
        if self.config.distance_metric != ho.COSINE:
            return super()._dist_pairs(a_id, ids)
        h = np.array([co.hamming(self.words[a_id], self.words[i]) for i in ids], dtype=np.int64)
        sim = F(1.0) - (h.astype(F) / F(self.dim))           # similarity(): hamming <= dim < 2^24, `as f32` is exact
        return (F(1.0) - sim).astype(F)

    def get_vector(self, node):
        return to_dense(self.words[node], self.dim)

    def memory_bytes(self):
        return self.n * 8 * self.words.shape[1] if self.n else 0


def build(rows, config=None, threshold="sign"):
    idx = HNSWBinIndex(config, threshold)
    for r in np.asarray(rows, dtype=F):
        idx.insert(r)
    return idx


# ---- tests/golden/hnsw_bin_small.npz (written by tests/golden/make_golden_hnsw_bin.py) ----------------------------------------
GOLDEN_K, GOLDEN_EF = 10, 50
GOLDEN_THRESHOLDS = ("sign", "median")
GOLDEN_METRICS = (ho.COSINE, ho.EUCLIDEAN, ho.DOT_PRODUCT)


def golden_case(rows, queries, t, metric):
    """the arrays of one (threshold, metric) pair, computed from scratch; keys carry the prefix `<threshold>_<metric>_`"""
    idx = build(rows, ho.HNSWConfig().with_distance_metric(metric), t)
    l0, l0cnt, up_head, up_ids = ho.golden_lists(idx)
    ids, sc, cnt = ho.padded_answers(idx, queries, GOLDEN_K, GOLDEN_EF)
    p = f"{t}_{metric}_"
    return {p + "levels": np.asarray(idx.levels, dtype=np.int64), p + "entry_point": np.int64(idx.entry_point),
            p + "max_layer": np.int64(idx.max_layer), p + "l0": l0.astype(np.int16), p + "l0cnt": l0cnt, p + "up_head": up_head,
            p + "up_ids": up_ids, p + "ids": ids, p + "scores": sc, p + "counts": cnt}


def golden_arrays():
    """every array of the golden file, computed from scratch"""
    rows, queries = ho.golden_corpus()
    out = {"rows": rows, "queries": queries, "k": np.int64(GOLDEN_K), "ef": np.int64(GOLDEN_EF)}
    for t in GOLDEN_THRESHOLDS:
        out[f"words_{t}"] = co.from_dense_rows(rows, t)
        for metric in GOLDEN_METRICS:
            out.update(golden_case(rows, queries, t, metric))
    return out
