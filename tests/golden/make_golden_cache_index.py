#!/usr/bin/env python3
"""Writes tests/golden/cache_index_small.npz from tests/_cache_index_oracle.py ALONE (never from the library).

A CacheIndex under the default config (Cosine walk): 400 inserts of 20 dimensions, every second one Sparse (70 % of its elements
zeroed, the others doubled), a tenth of the Sparse ones with a duplicated position; inserts 360 .. 399 RE-INSERT the keys 0 .. 39 (their
first nodes stay live: orphans), then the keys 40 .. 79 are removed (their nodes go dead).  64 dense and 64 sparse queries, 16 of the
sparse ones with a duplicated position; k in {1, 4, 10}; the nine metrics, Composite at its default weights.  The threshold of a
(metric, query) is the midpoint between two neighbouring similarities of the query's first ten LIVE candidates.

The generator asserts what a test could otherwise hide behind: of the 9 x 128 x 3 answers at least a quarter lose a candidate to the
threshold, at least a quarter lose one to the mask, at least a quarter differ (ids or score bits) from the re-rank of the to_dense()
rows (and the to_dense() query) under the max(2k, 10) rule; and for Angular / Geodesic every threshold lies at least 2^-20 (relative) from every candidate
similarity and no two live candidates of a query are closer than that, so that one ulp of acos can neither flip a comparison nor
reorder a tie.

    python tests/golden/make_golden_cache_index.py
"""
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests import _cache_index_oracle as co  # noqa: E402
from tests import _hnsw_mixed_oracle as mo  # noqa: E402
from tests import _xmetric_oracle as xo  # noqa: E402

F = np.float32
N, DIM, NQ = 400, 20, 64
KS = (1, 4, 10)
METRICS = [xo.Metric(k) for k in range(8)] + [xo.Metric(xo.COMPOSITE, xo.GeometricConfig.default())]
ACOS = (xo.ANGULAR, xo.GEODESIC)
SEP = 2.0 ** -20


def corpus():
    rng = np.random.default_rng(0xCAC4E)
    rows = rng.standard_normal((N, DIM)).astype(F)
    sparse = np.arange(N) % 2 == 1
    rows[sparse] = mo.sparsify(rng, rows[sparse], 0.7) * F(2.0)
    nodes = []
    for i in range(N):
        if not sparse[i]:
            nodes.append(None)
            continue
        sv = mo.SparseVector.from_dense(rows[i])
        if (i // 2) % 10 == 3 and len(sv):   # a tenth of the Sparse nodes: one stored position once more, with another value
            p = sv.positions[int(rng.integers(len(sv)))]
            sv = mo.SparseVector.from_parts(DIM, sv.positions + [p], np.append(sv.values, F(rng.standard_normal())))
        nodes.append(sv)
        rows[i] = sv.to_dense()
    keys = np.concatenate([np.arange(360), np.arange(40)]).astype(np.int32)
    removed = np.arange(40, 80, dtype=np.int32)
    return rows, nodes, keys, removed, rng


def draw_dense(rng, i):
    return rng.standard_normal(DIM).astype(F)


def draw_sparse(rng, i):
    while True:
        s = mo.SparseVector.from_dense(mo.sparsify(rng, rng.standard_normal((1, DIM)).astype(F), 0.6)[0])
        if len(s) >= 2:
            break
    if i % 4 == 1:                            # 16 of the 64
        p = s.positions[int(rng.integers(len(s)))]
        s = mo.SparseVector.from_parts(DIM, s.positions + [p], np.append(s.values, F(rng.standard_normal())))
    return s


def acos_separated(idx, live, form, query):
    """the Angular similarities (Geodesic's are the same) of the query's 30 candidates that are live: pairwise 4 x 2^-20 apart"""
    if form == "dense":
        cands, ent = [n for n, _ in idx.search(query, 30)], xo.Sparse(query)
    else:
        cands, ent = [n for n, _ in idx.search_sparse_with_ef(query, 30, idx.config.ef_search)], co.Entries(query)
    metric = xo.Metric(xo.ANGULAR)
    v = sorted(float(co.similarity(metric, ent, co.stored_entries(idx, n))) for n in cands if live[n])
    return all(b - a >= 4 * SEP * max(abs(a), abs(b)) for a, b in zip(v, v[1:]))


def queries(idx, live, rng):
    """drawn one by one; a draw whose candidates come too close under acos is drawn again"""
    out = {"dense": [], "sparse": []}
    redrawn = 0
    for form, draw in (("dense", draw_dense), ("sparse", draw_sparse)):
        for i in range(NQ):
            while True:
                q = draw(rng, i)
                if acos_separated(idx, live, form, q):
                    break
                redrawn += 1
            out[form].append(q)
    print(f"{redrawn} queries drawn again for the acos separation")
    return np.stack(out["dense"]), out["sparse"]


def build(rows, nodes, keys, removed):
    c = co.CacheIndex(DIM)
    for i in range(N):
        key = f"k{keys[i]}"
        got = c.insert(key, rows[i]) if nodes[i] is None else c.insert_sparse(key, nodes[i])
        assert got == i
    for k in removed:
        assert c.remove(f"k{k}")
    return c


def main():
    t = time.time()
    rows, nodes, keys, removed, rng = corpus()
    c = build(rows, nodes, keys, removed)
    idx = c.index
    live = np.array([i in c.node_to_key for i in range(N)])
    dq, sq = queries(idx, live, rng)
    assert sum(s.has_duplicates() for s in sq) == 16
    assert len(c) == 320 and live.sum() == 360
    dense_twin = [xo.Sparse(rows[i]) for i in range(N)]
    out = {"rows": rows, "sparse_mask": np.array([s is not None for s in nodes]), "keys": keys, "removed": removed, "live": live,
           "dense_queries": dq}
    out["node_indptr"], out["node_pos"], out["node_val"] = mo.csr_of([s for s in nodes if s is not None])
    out["sq_indptr"], out["sq_pos"], out["sq_val"] = mo.csr_of(sq)
    n_answers = n_thr = n_mask = n_differ = 0
    for form in ("dense", "sparse"):
        qents = [xo.Sparse(q) for q in dq] if form == "dense" else [co.Entries(s) for s in sq]
        qtwin = qents if form == "dense" else [xo.Sparse(s.to_dense()) for s in sq]   # what a dense-only re-rank would be given
        walks = {}
        for qi in range(NQ):
            for cc in sorted({co.candidate_count(k) for k in KS} | {xo.candidate_count(k) for k in KS}):
                if form == "dense":
                    walks[qi, cc] = [nid for nid, _ in idx.search(dq[qi], cc)]
                else:
                    walks[qi, cc] = [nid for nid, _ in idx.search_sparse_with_ef(sq[qi], cc, idx.config.ef_search)]
        thr = np.zeros((len(METRICS), NQ), dtype=F)
        differ = np.zeros((len(METRICS), NQ, len(KS)), dtype=bool)
        ans = {k: (np.full((len(METRICS), NQ, k), -1, dtype=np.int32), np.full((len(METRICS), NQ, k), -np.inf, dtype=F),
                   np.zeros((len(METRICS), NQ), dtype=np.uint8)) for k in KS}
        for mi, metric in enumerate(METRICS):
            sims, twin = {}, {}
            for qi in range(NQ):
                for node in walks[qi, 30]:
                    sims[qi, node] = co.similarity(metric, qents[qi], co.stored_entries(idx, node))
                    twin[qi, node] = co.similarity(metric, qtwin[qi], dense_twin[node])
                first = sorted({float(sims[qi, n]) for n in walks[qi, 10] if live[n]}, reverse=True)
                r = min(1 + qi % 3, len(first) - 2)
                thr[mi, qi] = F((first[r] + first[r + 1]) / 2.0)
                if metric.kind in ACOS:
                    t32 = float(thr[mi, qi])
                    vals = [float(sims[qi, n]) for n in walks[qi, 30] if live[n]]
                    assert all(abs(v - t32) >= SEP * max(abs(v), abs(t32)) for v in vals), (metric, qi)
                    sv = sorted(set(vals))
                    assert all(b - a >= SEP * abs(b) for a, b in zip(sv, sv[1:])), (metric, qi)
                    assert len(sv) == len(vals), (metric, qi, "a tie under acos")
                for k in KS:
                    cands = walks[qi, co.candidate_count(k)]
                    res = co.rescore(idx, lambda n: bool(live[n]), cands, qents[qi], k, thr[mi, qi], metric)
                    want = [(n, sims[qi, n]) for n in cands if live[n] and sims[qi, n] >= thr[mi, qi]]
                    want.sort(key=lambda e: -float(e[1]))
                    assert [(n, float(s)) for n, s in res] == [(n, float(s)) for n, s in want[:k]]
                    ids, sc, cnt = ans[k]
                    cnt[mi, qi] = len(res)
                    for j, (n, s) in enumerate(res):
                        ids[mi, qi, j] = n
                        sc[mi, qi, j] = s
                    alt = [(n, twin[qi, n]) for n in walks[qi, xo.candidate_count(k)] if live[n] and twin[qi, n] >= thr[mi, qi]]
                    alt.sort(key=lambda e: -float(e[1]))
                    alt = alt[:k]
                    n_answers += 1
                    n_thr += any(live[n] and not sims[qi, n] >= thr[mi, qi] for n in cands)
                    n_mask += any(not live[n] for n in cands)
                    differ[mi, qi, KS.index(k)] = [(n, F(s).tobytes()) for n, s in res] != [(n, F(s).tobytes()) for n, s in alt]
                    n_differ += int(differ[mi, qi, KS.index(k)])
        out[f"{form}_thresholds"] = thr
        out[f"{form}_differ"] = differ   # per (metric, query, k): the answer differs from the to_dense() / max(2k, 10) re-rank
        for k in KS:
            out[f"{form}_k{k}_ids"], out[f"{form}_k{k}_sims"], out[f"{form}_k{k}_counts"] = ans[k]
    print(f"{n_answers} answers: {n_thr} lose a candidate to the threshold, {n_mask} to the mask, {n_differ} differ from the "
          f"to_dense() / max(2k, 10) re-rank")
    assert 4 * n_thr >= n_answers and 4 * n_mask >= n_answers and 4 * n_differ >= n_answers
    out["n_differ"] = n_differ
    path = os.path.join(HERE, "cache_index_small.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {os.path.getsize(path)} bytes, {time.time() - t:.1f} s")


if __name__ == "__main__":
    main()
