#!/usr/bin/env python3
"""Write tests/golden/tt_decompose_small.npz: the twin's (tests/_tt_decompose_oracle.py) decompositions of the small cases of the
GPU list (dimension <= 128) and one Gaussian matrix — data only.  tests/test_tt_decompose_cpu.py holds the twin to it.

    python tools/make_tt_decompose_golden.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import _tt_decompose_oracle as do  # noqa: E402

out = {}
for name, shape, r, t, vectors in do.gpu_cases():
    if vectors.shape[1] > 128:
        continue
    status, ranks, off, cores = do.decompose_batch(vectors, shape, r, t)
    out.update({name + "_vectors": vectors, name + "_status": status, name + "_ranks": ranks, name + "_core_off": off,
                name + "_cores": cores})
out["gaussian_34x9_seed_1057"] = do.gaussian_matrix(34, 9, 33 * 31 + 34)
path = os.path.join(ROOT, "tests", "golden", "tt_decompose_small.npz")
np.savez_compressed(path, **out)
print(path, os.path.getsize(path), "bytes")
