#!/usr/bin/env python3
"""Writes tests/golden/hnsw_small.npz from tests/_hnsw_oracle.py ALONE (never from the library): rows, config, the level of
every node, every neighbour list, entry point, maximum layer, and the answers of a query set.

    python tests/golden/make_golden_hnsw.py

800 nodes x 20 elements (not a multiple of 8: the scalar tail takes part), HNSWConfig::default, cosine.  One node in eight is
an exact duplicate of an earlier one, so equal distances occur in the build and in the answers.  The pure-Python build took 6 s on
the CPU-only machine it was generated on.
"""
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests import _hnsw_oracle as ho  # noqa: E402

K, EF2 = 10, 120
corpus, lists = ho.golden_corpus, ho.golden_lists


def main():
    rows, queries = corpus()
    t = time.time()
    idx = ho.build(rows)
    took = time.time() - t
    l0, l0cnt, up_head, up_ids = lists(idx)
    ids, sc, cnt = ho.padded_answers(idx, queries, K)
    ids2, sc2, cnt2 = ho.padded_answers(idx, queries, K, ef=EF2)
    cfg = idx.config
    out = os.path.join(HERE, "hnsw_small.npz")
    np.savez_compressed(out, rows=rows, queries=queries, k=K, ef2=EF2,
                        config=np.asarray([cfg.m, cfg.m0, cfg.ef_construction, cfg.ef_search, cfg.distance_metric], dtype=np.int64),
                        levels=np.asarray(idx.levels, dtype=np.int32), entry_point=idx.entry_point, max_layer=idx.max_layer,
                        l0=l0, l0cnt=l0cnt, up_head=up_head, up_ids=up_ids, ids=ids, scores=sc, counts=cnt, ids_ef2=ids2,
                        scores_ef2=sc2, counts_ef2=cnt2)
    print(f"{out}: {os.path.getsize(out)} bytes, oracle build {took:.1f} s, max layer {idx.max_layer}, entry {idx.entry_point}")


if __name__ == "__main__":
    main()
