#!/usr/bin/env python3
"""Writes tests/golden/hnsw_tt_small.npz from tests/_hnsw_tt_oracle.py ALONE (never from the library): the 800 x 20 corpus of
_hnsw_oracle.golden_corpus() built under Cosine, Euclidean and DotProduct with the default config, and 64 tensor-train queries of
shape [2,2,5], ranks [1,2,2,1] (golden_trains()): their cores, reconstructions and norms, and per index the answers of
search_tt_with_ef at k 10, ef 50, the answers of search_with_ef to the RECONSTRUCTED query, and the number of queries whose ids or
score bits differ between the two — what makes a TT search more than "densify and search".

    python tests/golden/make_golden_hnsw_tt.py
"""
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests import _hnsw_oracle as ho  # noqa: E402
from tests import _hnsw_tt_oracle as to  # noqa: E402


def main():
    rows, _ = ho.golden_corpus()
    tts = to.golden_trains()
    shape, ranks, off, cores = to.pack(tts)
    recon = np.stack([to.tt_reconstruct(t) for t in tts])
    norms = np.asarray([to.tt_norm(t) for t in tts], dtype=np.float32)
    mags = np.asarray([ho.magnitude(r) for r in recon], dtype=np.float32)
    out = {"shape": shape, "ranks": ranks, "core_off": off, "cores": cores, "reconstructions": recon, "norms": norms,
           "norms_differ": int((norms.view(np.uint32) != mags.view(np.uint32)).sum())}
    print(f"{out['norms_differ']} of {len(tts)} norms differ in bits from simd::magnitude of the reconstruction")
    t = time.time()
    for name, metric in (("cosine", ho.COSINE), ("euclidean", ho.EUCLIDEAN), ("dot", ho.DOT_PRODUCT)):
        idx = ho.build(rows, ho.HNSWConfig().with_distance_metric(metric))
        ids, sc, cnt = to.answers_tt(idx, tts, 10, 50)
        dids, dsc, _ = ho.padded_answers(idx, recon, 10, 50)
        differ = int(((ids != dids) | (sc.view(np.uint32) != dsc.view(np.uint32))).any(axis=1).sum())
        print(f"{name}: {differ} of {len(tts)} answers differ from search of the reconstructed query")
        out.update({f"{name}_ids": ids, f"{name}_scores": sc, f"{name}_counts": cnt, f"{name}_differ": differ})
    path = os.path.join(HERE, "hnsw_tt_small.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {os.path.getsize(path)} bytes, oracle builds {time.time() - t:.1f} s")


if __name__ == "__main__":
    main()
