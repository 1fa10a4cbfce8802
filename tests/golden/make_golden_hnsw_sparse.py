#!/usr/bin/env python3
"""Writes tests/golden/hnsw_small_sparse.npz from tests/_hnsw_oracle.py ALONE (never from the library): the graph the oracle
builds over tests/_xmetric_oracle.sparse_golden_corpus() — golden_corpus() with 60 % of the entries zeroed — in the layout of
hnsw_small.npz (rows, queries, config, levels, neighbour lists, entry point, maximum layer).

    python tests/golden/make_golden_hnsw_sparse.py

The pure-Python build took 10 s on the CPU-only machine it was generated on; tests/test_gpu_xmetric.py reads the graph back
instead of building it, and holds the graph nmn_hnsw_insert builds over the same rows to it."""
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests import _hnsw_oracle as ho  # noqa: E402
from tests import _xmetric_oracle as xo  # noqa: E402


def main():
    rows, queries = xo.sparse_golden_corpus()
    t = time.time()
    idx = ho.build(rows)
    took = time.time() - t
    l0, l0cnt, up_head, up_ids = ho.golden_lists(idx)
    cfg = idx.config
    out = os.path.join(HERE, "hnsw_small_sparse.npz")
    np.savez_compressed(out, rows=rows, queries=queries,
                        config=np.asarray([cfg.m, cfg.m0, cfg.ef_construction, cfg.ef_search, cfg.distance_metric], dtype=np.int64),
                        levels=np.asarray(idx.levels, dtype=np.int32), entry_point=idx.entry_point, max_layer=idx.max_layer,
                        l0=l0, l0cnt=l0cnt, up_head=up_head, up_ids=up_ids)
    print(f"{out}: {os.path.getsize(out)} bytes, oracle build {took:.1f} s, max layer {idx.max_layer}, entry {idx.entry_point}")


if __name__ == "__main__":
    main()
