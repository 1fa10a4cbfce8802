#!/usr/bin/env python3
"""Writes tests/golden/hnsw_bin_small.npz from tests/_hnsw_bin_oracle.py ALONE (never from the library): the corpus of
hnsw_small.npz (800 x 20, one node in eight a duplicate) with every node EmbeddingStorage::Binary — for BinaryThreshold::Sign and
::Median the words of every row, and for each of them under Cosine, Euclidean and DotProduct the level of every node, every
neighbour list, entry point, maximum layer and the answers of the 64 queries at k 10, ef 50.

    python tests/golden/make_golden_hnsw_bin.py

HNSWConfig::default.  The six pure-Python builds take about a minute.
"""
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests import _hnsw_bin_oracle as hb  # noqa: E402


def main():
    t = time.time()
    arrays = hb.golden_arrays()
    took = time.time() - t
    out = os.path.join(HERE, "hnsw_bin_small.npz")
    np.savez_compressed(out, **arrays)
    print(f"{out}: {os.path.getsize(out)} bytes, {len(arrays)} arrays, oracle builds {took:.1f} s")


if __name__ == "__main__":
    main()
