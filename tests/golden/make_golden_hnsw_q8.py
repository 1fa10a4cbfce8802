#!/usr/bin/env python3
"""Writes tests/golden/hnsw_q8_small.npz from tests/_hnsw_q8_oracle.py ALONE (never from the library): the corpus of
hnsw_small.npz (800 x 20, one node in eight a duplicate) indexed with HNSWStorageStrategy::Quantized — every row's codes, scale,
min_val and dequantized vector, the level of every node, every neighbour list, entry point, maximum layer, and the answers of
the query set with their evaluation counts.

    python tests/golden/make_golden_hnsw_q8.py

HNSWConfig::default, cosine.  The pure-Python build takes some ten seconds.
"""
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests import _hnsw_oracle as ho  # noqa: E402
from tests import _hnsw_q8_oracle as q8  # noqa: E402


def main():
    rows, queries = ho.golden_corpus()
    t = time.time()
    idx = q8.build(rows)
    took = time.time() - t
    l0, l0cnt, up_head, up_ids = ho.golden_lists(idx)
    K, EF2 = q8.GOLDEN_K, q8.GOLDEN_EF2
    ids, sc, cnt = ho.padded_answers(idx, queries, K)
    ids2, sc2, cnt2 = ho.padded_answers(idx, queries, K, ef=EF2)
    cfg = idx.config
    n = idx.n
    out = os.path.join(HERE, "hnsw_q8_small.npz")
    np.savez_compressed(out, rows=rows, queries=queries, k=K, ef2=EF2,
                        config=np.asarray([cfg.m, cfg.m0, cfg.ef_construction, cfg.ef_search, cfg.distance_metric], dtype=np.int64),
                        codes=idx.codes[:n], scale=idx.scale[:n], min_val=idx.min_val[:n], dequantized=idx.rows[:n],
                        levels=np.asarray(idx.levels, dtype=np.int32), entry_point=idx.entry_point, max_layer=idx.max_layer,
                        l0=l0, l0cnt=l0cnt, up_head=up_head, up_ids=up_ids, ids=ids, scores=sc, counts=cnt, ids_ef2=ids2,
                        scores_ef2=sc2, counts_ef2=cnt2)
    print(f"{out}: {os.path.getsize(out)} bytes, oracle build {took:.1f} s, max layer {idx.max_layer}, entry {idx.entry_point}")


if __name__ == "__main__":
    main()
