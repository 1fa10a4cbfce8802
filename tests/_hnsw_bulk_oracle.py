"""CPU restatement of the batched HNSW build (docs/hnsw.md §19) over tests/_hnsw_oracle.py — TEST INFRASTRUCTURE ONLY.

Written from the scheme's description, not from neumann_amd/csrc/nmn_hnsw.hip:

  1. the levels of all rows of a call are drawn first, in order (random_level, hnsw.rs:1631-1651);
  2. the first node of an empty index, and every node while the graph holds fewer than `min_nodes`, is inserted the plain way;
  3. a batch is the next B nodes, cut behind the first one whose level exceeds max_layer as it is when the batch starts;
  4. every node of the batch is WALKED against the graph as it is when the batch starts (greedy descent above its level, then
     search_layer with ef_construction on every layer from min(level, max_layer) down), the (node, layer) lists it reads recorded;
  5. the nodes are COMMITTED in order.  A commit assigns the new node's list on every searched layer and the list of every
     selected neighbour there, pruned or not; all of these become dirty.  A walk is accepted iff it read no dirty list; otherwise
     the node is walked again against the graph as it is now.  Either way all of a node's searches come before its commits.

`bulk_build(..., validate=False)` accepts every walk: the broken scheme the tests must be able to tell from the right one.
"""
import functools

import numpy as np

from tests import _hnsw_oracle as ho

F = np.float32


# ---- the walk, over `lst(node, layer)` ---------------------------------------------------------------------------------------------
def _greedy(idx, q, qmag, entry, layer, lst):
    current = entry
    current_dist = float(idx._dist_query([current], q, qmag)[0])
    while True:
        ids = lst(current, layer)
        changed = False
        if ids:
            ds = idx._dist_query(ids, q, qmag)
            for nid, d in zip(ids, ds.tolist()):
                if d < current_dist:
                    current, current_dist, changed = nid, d, True
        if not changed:
            return current


def _search_layer(idx, q, qmag, entry, ef, layer, lst):
    visited = {entry}
    candidates = ho.BinaryHeap(ho.neighbor_le)
    results = ho.BinaryHeap(ho.max_neighbor_le)
    d0 = float(idx._dist_query([entry], q, qmag)[0])
    candidates.push((d0, entry))
    results.push((d0, entry))
    while True:
        current = candidates.pop()
        if current is None:
            break
        if len(results) >= ef and current[0] > results.peek()[0]:
            break
        fresh = []
        for nid in lst(current[1], layer):      # (the list of a popped candidate that passed the termination test: a read)
            if nid not in visited:
                visited.add(nid)
                fresh.append(nid)
        if not fresh:
            continue
        for nid, dist in zip(fresh, idx._dist_query(fresh, q, qmag).tolist()):
            if len(results) < ef or dist < results.peek()[0]:
                candidates.push((dist, nid))
                results.push((dist, nid))
                while len(results) > ef:
                    results.pop()
    vec = results.into_vec()
    vec.sort(key=lambda e: e[0])
    return vec


def walk(idx, q, level, reads=None):
    """every search of one insert against idx as it is now -> {layer: selected ids}; `reads` collects the (node, layer) read"""
    cfg = idx.config

    def lst(node, layer):
        if reads is not None:
            reads.add((node, layer))
        return idx.neighbors[node][layer]

    qmag = idx._qmag(q)
    cur = idx.entry_point
    for layer in range(idx.max_layer, level, -1):
        cur = _greedy(idx, q, qmag, cur, layer, lst)
    selected = {}
    for layer in range(min(level, idx.max_layer), -1, -1):
        found = _search_layer(idx, q, qmag, cur, cfg.ef_construction, layer, lst)
        m = cfg.m0 if layer == 0 else cfg.m
        selected[layer] = [e[1] for e in found[:m]]
        if found:
            cur = found[0][1]
    return selected


# ---- the commit ----------------------------------------------------------------------------------------------------------------------
def _add_node(idx, v, level):
    node = idx.n
    if idx.rows is None:
        idx.rows = np.zeros((64, v.size), dtype=F)
        idx.mags = np.zeros(64, dtype=F)
    while node >= idx.rows.shape[0]:
        idx.rows = np.concatenate([idx.rows, np.zeros_like(idx.rows)])
        idx.mags = np.concatenate([idx.mags, np.zeros_like(idx.mags)])
    idx.rows[node] = v
    idx.mags[node] = ho.magnitude(v)
    idx.n += 1
    idx.levels.append(level)
    idx.neighbors.append([[] for _ in range(level + 1)])
    return node


def commit(idx, node, level, selected, dirty):
    """hnsw.rs:2005-2050 for every searched layer, top down; every list assigned goes into `dirty`"""
    cfg = idx.config
    current_max = idx.max_layer
    for layer in range(min(level, current_max), -1, -1):
        m = cfg.m0 if layer == 0 else cfg.m
        sel = selected[layer]
        idx.neighbors[node][layer] = sorted(idx.neighbors[node][layer] + sel)
        dirty.add((node, layer))
        for nb in sel:
            lst = sorted(idx.neighbors[nb][layer] + [node])
            if len(lst) > m:
                ds = idx._dist_pairs(nb, lst).tolist()
                lst = sorted(t[0] for t in sorted(zip(lst, ds), key=lambda t: t[1])[:m])
            idx.neighbors[nb][layer] = lst
            dirty.add((nb, layer))
    if level > current_max:
        idx.entry_point = node
        idx.max_layer = level


def bulk_insert(idx, rows, batch, min_nodes=1, validate=True):
    """insert `rows` into idx by the scheme above -> {batches, walks, accepted, conflicts, host_nodes}"""
    rows = np.asarray(rows, dtype=F)
    levels = [idx.random_level() for _ in rows]
    st = dict(batches=0, walks=0, accepted=0, conflicts=0, host_nodes=0)
    i, n = 0, len(rows)
    while i < n and (idx.entry_point is None or idx.n < max(min_nodes, 1)):
        if idx.entry_point is None:
            idx.entry_point = _add_node(idx, rows[i], levels[i])
            idx.max_layer = levels[i]
        else:
            sel = walk(idx, rows[i], levels[i])
            commit(idx, _add_node(idx, rows[i], levels[i]), levels[i], sel, set())
        st["host_nodes"] += 1
        i += 1
    while i < n:
        nb = min(batch, n - i)
        for j in range(nb):
            if levels[i + j] > idx.max_layer:
                nb = j + 1
                break
        spec = []
        for j in range(nb):                      # all walks of the batch see the graph before any of its commits
            reads = set()
            spec.append((walk(idx, rows[i + j], levels[i + j], reads), reads))
        dirty = set()
        for j in range(nb):
            sel, reads = spec[j]
            if validate and reads & dirty:
                st["conflicts"] += 1
                sel = walk(idx, rows[i + j], levels[i + j])
            else:
                st["accepted"] += 1
            commit(idx, _add_node(idx, rows[i + j], levels[i + j]), levels[i + j], sel, dirty)
        st["batches"] += 1
        st["walks"] += nb
        i += nb
    return st


def bulk_build(rows, config, batch, min_nodes=1, validate=True):
    idx = ho.HNSWIndex(config)
    return idx, bulk_insert(idx, rows, batch, min_nodes, validate)


def same_graph(a, b):
    return (a.n == b.n and a.levels == b.levels and a.entry_point == b.entry_point and a.max_layer == b.max_layer
            and a.rng_seed == b.rng_seed and a.neighbors == b.neighbors)


# ---- the corpora of the tests ------------------------------------------------------------------------------------------------------
# name -> (kind, n, dim, m, ef_construction, metric, batch)
CASES = {
    "plain-cos": ("plain", 1200, 24, 8, 16, ho.COSINE, 8),
    "dup-eucl": ("dup", 1200, 24, 8, 16, ho.EUCLIDEAN, 8),
    "plain-dot-b32": ("plain", 1200, 24, 4, 8, ho.DOT_PRODUCT, 32),
    "same-cos": ("same", 150, 9, 8, 16, ho.COSINE, 8),
    "plain-default": ("plain", 360, 20, 16, 200, ho.COSINE, 8),
}


def make_rows(kind, n, d, seed):
    """clustered rows; "dup": a quarter of them exact duplicates of earlier ones; "same": identical rows only"""
    rng = np.random.default_rng(seed)
    rows = (rng.standard_normal((n, d)) + 2.0 * rng.standard_normal((6, d))[rng.integers(0, 6, n)]).astype(F)
    if kind == "dup":
        for i in range(4, n, 4):
            rows[i] = rows[rng.integers(0, i)]
    elif kind == "same":
        rows[:] = rows[0]
    return rows


def case_config(name):
    _, _, _, m, efc, metric, _ = CASES[name]
    return ho.HNSWConfig(m=m, ef_construction=efc, distance_metric=metric)


@functools.lru_cache(maxsize=None)
def case_rows(name):
    kind, n, d = CASES[name][:3]
    rows = make_rows(kind, n, d, 0xB01C + sum(map(ord, name)))
    rows.setflags(write=False)
    return rows


@functools.lru_cache(maxsize=None)
def case_sequential(name):
    """the reference's graph: one insert after the other"""
    return ho.build(case_rows(name), case_config(name))


@functools.lru_cache(maxsize=None)
def case_bulk(name, validate=True):
    """-> (index, counts) of the batched build at the case's batch size, min_nodes 1"""
    return bulk_build(case_rows(name), case_config(name), CASES[name][6], 1, validate)
