"""CPU restatement of the reference's HNSW index with dense storage — TEST INFRASTRUCTURE ONLY.

The product builds the graph in neumann_amd/csrc/nmn_hnsw.hip (host C++) and walks it in a HIP kernel; this file is written
from the reference's text independently of both (paths relative to the reference root):
  tensor_store/src/hnsw.rs   HNSWDistanceMetric::to_similarity 152-158, simd::dot_product 168-193, sum_of_squares / magnitude
                             198-229, euclidean_distance 234-261 (the 8-lane form), cosine / euclidean / dot_product
                             _distance_dense 1035-1045 / 1084-1086 / 1136-1138, distance_dense 1157-1163,
                             CompressedNeighbors::set (sorted ids) 1306-1314, Neighbor / MaxNeighbor 1380-1430,
                             HNSWConfig and its presets 1434-1551, next_random / random_level 1631-1651,
                             try_insert_embedding 1936-2051, search_with_ef 2069-2111, search_layer_greedy 2170-2200,
                             search_layer 2276-2335, try_cosine / euclidean / dot_product_distance (Dense pairs) 2437-2452 ff.
  vector_engine/src/lib.rs   build_hnsw_index 2378-2470, estimate_hnsw_memory 2489-2509, search_with_hnsw 2516-2550

`BinaryHeap` is std::collections::BinaryHeap as an array algorithm (push: append, sift_up(0, old_len); pop: Vec::pop, swap with
the root, sift_down_to_bottom(0) — the hole goes to the bottom following the greater child, the RIGHT one when the two compare
equal because the test is `hole.get(child) <= hole.get(child + 1)` — then sift_up; into_iter: the vector's order).  Neighbor and
MaxNeighbor compare by distance ALONE, so that layout decides every tie.  The description is the standard library's published
algorithm restated from memory (its source is not part of the reference); tie order is pinned by restatement only.

Every f32 sum is an explicit sequence of numpy float32 operations (each rounded once, never fused; np.sum is pairwise and would
round differently).  Distances are evaluated for a batch of rows at a time — the order INSIDE each row's chains is the reference's.
"""
import math

import numpy as np

F = np.float32
COSINE, EUCLIDEAN, DOT_PRODUCT = 0, 1, 2
U64 = (1 << 64) - 1


class HNSWConfig:
    def __init__(self, m=16, m0=None, ef_construction=200, ef_search=50, ml=None, sparsity_threshold=0.5, max_nodes=10_000_000,
                 distance_metric=COSINE):
        self.m = m
        self.m0 = 2 * m if m0 is None else m0
        self.ef_construction = ef_construction
        self.ef_search = ef_search
        self.ml = 1.0 / math.log(float(m)) if ml is None else ml
        self.sparsity_threshold = sparsity_threshold
        self.max_nodes = max_nodes
        self.distance_metric = distance_metric

    @staticmethod
    def high_recall():
        return HNSWConfig(m=32, m0=64, ef_construction=400, ef_search=200, ml=1.0 / math.log(32.0))

    @staticmethod
    def high_speed():
        return HNSWConfig(m=8, m0=16, ef_construction=100, ef_search=20, ml=1.0 / math.log(8.0))

    def with_distance_metric(self, metric):
        self.distance_metric = metric
        return self


class CapacityExceeded(Exception):
    def __init__(self, limit, current):
        super().__init__(f"HNSW index at capacity: {current} nodes (limit: {limit})")
        self.limit, self.current = limit, current


# ---- std::collections::BinaryHeap ---------------------------------------------------------------------------------------------
class BinaryHeap:
    """`le(a, b)` is `a <= b` under the element's Ord."""

    def __init__(self, le):
        self.data = []
        self.le = le

    def __len__(self):
        return len(self.data)

    def peek(self):
        return self.data[0] if self.data else None

    def push(self, item):
        old_len = len(self.data)
        self.data.append(item)
        self._sift_up(0, old_len)

    def pop(self):
        d = self.data
        if not d:
            return None
        item = d.pop()
        if d:
            item, d[0] = d[0], item
            self._sift_down_to_bottom(0)
        return item

    def _sift_up(self, start, pos):
        d = self.data
        elt = d[pos]
        while pos > start:
            parent = (pos - 1) // 2
            if self.le(elt, d[parent]):
                break
            d[pos] = d[parent]
            pos = parent
        d[pos] = elt

    def _sift_down_to_bottom(self, pos):
        d = self.data
        end = len(d)
        start = pos
        elt = d[pos]
        child = 2 * pos + 1
        while child <= max(end - 2, 0) and end >= 2:
            if self.le(d[child], d[child + 1]):
                child += 1
            d[pos] = d[child]
            pos = child
            child = 2 * pos + 1
        if child == end - 1:
            d[pos] = d[child]
            pos = child
        d[pos] = elt
        self._sift_up(start, pos)

    def into_vec(self):
        return list(self.data)


# elements are (distance as a Python float holding the f32 value, id)
def neighbor_le(a, b):      # Neighbor::cmp = other.distance.partial_cmp(self.distance): a <= b iff b.distance <= a.distance
    return b[0] <= a[0]


def max_neighbor_le(a, b):  # MaxNeighbor::cmp = self.distance.partial_cmp(other.distance)
    return a[0] <= b[0]


# ---- simd::* in the reference's order, a batch of rows against one vector ----------------------------------------------------
def _lanes(A, q, square_of_difference):
    """the eight chains, their left-to-right sum from -0.0 and the scalar tail: r for every row of A"""
    A = np.asarray(A, dtype=F)
    q = np.asarray(q, dtype=F)
    r, dim = A.shape
    chunks = dim // 8
    acc = np.zeros((r, 8), dtype=F)
    for c in range(chunks):
        x = A[:, 8 * c:8 * c + 8]
        y = q[8 * c:8 * c + 8]
        if square_of_difference:
            d = x - y
            p = d * d
        else:
            p = x * y
        acc = acc + p
    res = np.full(r, -0.0, dtype=F)
    for lane in range(8):
        res = res + acc[:, lane]
    for i in range(chunks * 8, dim):
        if square_of_difference:
            d = A[:, i] - q[i]
            res = res + d * d
        else:
            res = res + A[:, i] * q[i]
    return res


def dot_product_rows(A, q):
    return _lanes(A, q, False)


def magnitude(v):
    v = np.asarray(v, dtype=F)
    return np.sqrt(_lanes(v[None, :], v, False))[0]


def euclidean_distance_rows(A, q):
    return np.sqrt(_lanes(A, q, True))


def to_similarity(metric, distance):
    d = F(distance)
    if metric == COSINE:
        return F(1.0) - d
    if metric == EUCLIDEAN:
        return F(1.0) / (F(1.0) + d)
    return -d


class HNSWIndex:
    def __init__(self, config=None):
        self.config = config or HNSWConfig()
        self.n = 0
        self.rows = None          # [capacity][dim] f32
        self.mags = None          # simd::magnitude of every row
        self.levels = []
        self.neighbors = []       # [node][layer] -> sorted list of ids
        self.entry_point = None   # usize::MAX
        self.max_layer = 0
        self.rng_seed = 42
        self.distance_evals = 0

    def __len__(self):
        return self.n

    # hnsw.rs:1631-1651
    def next_random(self):
        s = self.rng_seed
        s ^= (s << 13) & U64
        s ^= s >> 7
        s ^= (s << 17) & U64
        self.rng_seed = s
        return s

    def random_level(self):
        r = self.next_random()
        f = float(r) / float(U64)
        level = math.floor(-math.log(f) * self.config.ml)
        return min(int(level), 32)

    # distance_dense(stored rows `ids`, query)
    def _dist_query(self, ids, q, qmag):
        metric = self.config.distance_metric
        A = self.rows[ids]
        self.distance_evals += len(ids)
        if metric == EUCLIDEAN:
            return euclidean_distance_rows(A, q)
        dot = dot_product_rows(A, q)
        if metric == DOT_PRODUCT:
            return -dot
        mag_self = self.mags[ids]
        with np.errstate(divide="ignore", invalid="ignore"):
            d = F(1.0) - (dot / (mag_self * qmag))
        d[(mag_self == 0) | (qmag == 0)] = F(1.0)
        return d

    # try_cosine / euclidean / dot_product_distance on Dense pairs: a = the neighbour being pruned, b = rows `ids`
    def _dist_pairs(self, a_id, ids):
        metric = self.config.distance_metric
        va = self.rows[a_id]
        B = self.rows[ids]
        if metric == EUCLIDEAN:
            return euclidean_distance_rows(B, va)   # (a - b)^2 == (b - a)^2 bit for bit
        dot = dot_product_rows(B, va)               # a[i] * b[i] == b[i] * a[i]
        if metric == DOT_PRODUCT:
            return -dot
        mag_a = self.mags[a_id]
        mag_b = self.mags[ids]
        with np.errstate(divide="ignore", invalid="ignore"):
            d = F(1.0) - (dot / (mag_a * mag_b))
        d[(mag_b == 0) | (mag_a == 0)] = F(1.0)
        return d

    def _qmag(self, q):
        return magnitude(q) if self.config.distance_metric == COSINE else F(0)

    def search_layer_greedy(self, q, qmag, entry_id, layer):
        current = entry_id
        current_dist = float(self._dist_query([current], q, qmag)[0])
        while True:
            ids = self.neighbors[current][layer]
            changed = False
            if ids:
                ds = self._dist_query(ids, q, qmag)
                for nid, d in zip(ids, ds.tolist()):
                    if d < current_dist:
                        current, current_dist, changed = nid, d, True
            if not changed:
                break
        return current

    def search_layer(self, q, qmag, entry_id, ef, layer):
        visited = set()
        candidates = BinaryHeap(neighbor_le)
        results = BinaryHeap(max_neighbor_le)
        entry_dist = float(self._dist_query([entry_id], q, qmag)[0])
        visited.add(entry_id)
        candidates.push((entry_dist, entry_id))
        results.push((entry_dist, entry_id))
        while True:
            current = candidates.pop()
            if current is None:
                break
            if len(results) >= ef:
                worst = results.peek()
                if worst is not None and current[0] > worst[0]:
                    break
            fresh = []
            for nid in self.neighbors[current[1]][layer]:
                if nid not in visited:
                    visited.add(nid)
                    fresh.append(nid)
            if not fresh:
                continue
            ds = self._dist_query(fresh, q, qmag).tolist()
            for nid, dist in zip(fresh, ds):
                worst = results.peek()
                should_add = len(results) < ef or worst is None or dist < worst[0]
                if should_add:
                    candidates.push((dist, nid))
                    results.push((dist, nid))
                    while len(results) > ef:
                        results.pop()
        vec = results.into_vec()
        vec.sort(key=lambda e: e[0])  # slice::sort_by is stable, and so is list.sort
        return vec

    def insert(self, vector):
        cfg = self.config
        v = np.asarray(vector, dtype=F)
        if cfg.max_nodes > 0 and self.n >= cfg.max_nodes:
            raise CapacityExceeded(cfg.max_nodes, self.n)
        node_level = self.random_level()
        node_id = self.n
        if self.rows is None:
            self.rows = np.zeros((64, v.size), dtype=F)
            self.mags = np.zeros(64, dtype=F)
        if node_id == self.rows.shape[0]:
            self.rows = np.concatenate([self.rows, np.zeros_like(self.rows)])
            self.mags = np.concatenate([self.mags, np.zeros_like(self.mags)])
        self.rows[node_id] = v
        self.mags[node_id] = magnitude(v)
        self.n += 1
        self.levels.append(node_level)
        self.neighbors.append([[] for _ in range(node_level + 1)])
        current_max = self.max_layer
        entry_id = self.entry_point
        if entry_id is None:
            self.entry_point = node_id
            self.max_layer = node_level
            return node_id
        q = self.rows[node_id].copy()
        qmag = self._qmag(q)
        current_node = entry_id
        for layer in range(current_max, node_level, -1):
            current_node = self.search_layer_greedy(q, qmag, current_node, layer)
        for layer in range(min(node_level, current_max), -1, -1):
            found = self.search_layer(q, qmag, current_node, cfg.ef_construction, layer)
            m = cfg.m0 if layer == 0 else cfg.m
            selected = [e[1] for e in found[:m]]
            self.neighbors[node_id][layer] = sorted(self.neighbors[node_id][layer] + selected)
            for nb in selected:
                lst = sorted(self.neighbors[nb][layer] + [node_id])
                if len(lst) > m:
                    ds = self._dist_pairs(nb, lst).tolist()
                    with_dist = sorted(zip(lst, ds), key=lambda t: t[1])  # stable, over the id-ascending list
                    lst = sorted(t[0] for t in with_dist[:m])
                self.neighbors[nb][layer] = lst
            if found:
                current_node = found[0][1]
        if node_level > current_max:
            self.entry_point = node_id
            self.max_layer = node_level
        return node_id

    def search_with_ef(self, query, k, ef):
        """-> [(id, similarity f32)]"""
        if self.entry_point is None:
            return []
        q = np.asarray(query, dtype=F)
        qmag = self._qmag(q)
        current = self.entry_point
        for layer in range(self.max_layer, 0, -1):
            current = self.search_layer_greedy(q, qmag, current, layer)
        cand = self.search_layer(q, qmag, current, max(ef, k), 0)
        metric = self.config.distance_metric
        return [(nid, to_similarity(metric, d)) for d, nid in cand[:k]]

    def search(self, query, k):
        return self.search_with_ef(query, k, self.config.ef_search)


def build(rows, config=None):
    idx = HNSWIndex(config)
    for r in np.asarray(rows, dtype=F):
        idx.insert(r)
    return idx


def padded_answers(idx, queries, k, ef=None):
    """the library's output layout: ids u64 [nq][k] (unused = UINT64_MAX), scores f32 (unused = -inf), counts"""
    Q = np.asarray(queries, dtype=F)
    if Q.ndim == 1:
        Q = Q[None, :]
    ids = np.full((Q.shape[0], k), np.uint64(0xFFFFFFFFFFFFFFFF), dtype=np.uint64)
    sc = np.full((Q.shape[0], k), -np.inf, dtype=F)
    cnt = np.zeros(Q.shape[0], dtype=np.uint32)
    for i, q in enumerate(Q):
        res = idx.search_with_ef(q, k, idx.config.ef_search if ef is None else ef)
        cnt[i] = len(res)
        for j, (nid, s) in enumerate(res):
            ids[i, j] = nid
            sc[i, j] = s
    return ids, sc, cnt


# ---- vector_engine: estimate_hnsw_memory (lib.rs:2489-2509) and search_with_hnsw's key mapping (2516-2550) ----------------
def estimate_hnsw_memory(count, dim):
    """lib.rs:2489-2509: vectors count * dim * 4, graph count * 16 * 2 * 8 (M = 16 whatever the config), keys count * 32"""
    if count == 0:
        return 0
    return count * dim * 4 + count * 16 * 2 * 8 + count * 32


def search_with_hnsw(idx, key_mapping, query, top_k):
    """lib.rs:2516-2550 -> [(key, score)]; node ids past the mapping are dropped"""
    if len(query) == 0:
        raise ValueError("Empty vector provided")
    if top_k == 0:
        raise ValueError("Invalid top_k value (must be > 0)")
    return [(key_mapping[nid], s) for nid, s in idx.search(query, top_k) if nid < len(key_mapping)]


# ---- tests/golden/hnsw_small.npz (written by tests/golden/make_golden_hnsw.py, checked by tests/test_hnsw_oracle_cpu.py) --------
def golden_corpus(n=800, dim=20, nq=64):
    """800 x 20 (the scalar tail takes part), one node in eight an exact duplicate of an earlier one; queries 0-7 ARE rows"""
    rng = np.random.default_rng(0x4A5)
    rows = rng.standard_normal((n, dim)).astype(np.float32)
    for i in range(8, n, 8):
        rows[i] = rows[rng.integers(0, i)]
    queries = rng.standard_normal((nq, dim)).astype(np.float32)
    queries[:8] = rows[8:16]
    return rows, queries


def golden_lists(idx):
    """layer 0 as [n][m0] (-1 padded) + counts; upper layers as (node, layer, count) triples + the ids concatenated"""
    cfg = idx.config
    l0 = np.full((idx.n, cfg.m0), -1, dtype=np.int64)
    l0cnt = np.zeros(idx.n, dtype=np.int32)
    up_head, up_ids = [], []
    for node in range(idx.n):
        a = idx.neighbors[node][0]
        l0cnt[node] = len(a)
        l0[node, :len(a)] = a
        for layer in range(1, idx.levels[node] + 1):
            b = idx.neighbors[node][layer]
            up_head.append((node, layer, len(b)))
            up_ids.extend(b)
    return l0, l0cnt, np.asarray(up_head, dtype=np.int64).reshape(-1, 3), np.asarray(up_ids, dtype=np.int64)
