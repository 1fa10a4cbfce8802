#!/usr/bin/env python3
"""Writes tests/golden/tt_similarity_small.npz from tests/_tt_similarity_oracle.py ALONE (never from the library): 16 x 24 Gaussian
trains of shape [2,2,5] (golden_sets(): queries at ranks [1,2,2,1], every other target at ranks [1,2,3,1]), the three matrices
tt_dot_product, tt_cosine_similarity and tt_euclidean_distance, and two counts that make the comparison more than "reconstruct and
take the dense dot": the pairs whose dot differs in bits from simd::dot_product of the two reconstructions, and the pairs whose dot
differs in bits from the swapped pair's.  Also one pair whose squared Euclidean distance is negative before the clamp
(one_ulp_pairs()); the script fails if its own search finds none.

    python tests/golden/make_golden_tt_similarity.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests import _hnsw_oracle as ho  # noqa: E402
from tests import _hnsw_tt_oracle as to  # noqa: E402
from tests import _tt_similarity_oracle as so  # noqa: E402

F = np.float32


def bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


def main():
    qs, ts = so.golden_sets()
    _, rq, oq, cq = so.pack(qs)
    shape, rt, ot, ct = so.pack(ts)
    out = {"shape": shape, "ranks_q": rq, "core_off_q": oq, "cores_q": cq, "ranks_t": rt, "core_off_t": ot, "cores_t": ct}
    for name, op in (("dot", so.DOT), ("cosine", so.COSINE), ("euclidean", so.EUCLIDEAN)):
        out[name] = so.similarity(op, qs, ts)
    out["self_q"] = np.asarray([so.self_dot(t) for t in qs], dtype=F)
    out["self_t"] = np.asarray([so.self_dot(t) for t in ts], dtype=F)
    rec_t = np.stack([to.tt_reconstruct(t) for t in ts])
    dense = np.stack([ho.dot_product_rows(rec_t, to.tt_reconstruct(q)) for q in qs])
    swapped = so.similarity(so.DOT, ts, qs).T
    out["dense_differ"] = int((bits(out["dot"]) != bits(dense)).sum())
    out["swapped_differ"] = int((bits(out["dot"]) != bits(swapped)).sum())
    print(f"{out['dense_differ']} of {dense.size} dots differ in bits from the dense dot of the reconstructions")
    print(f"{out['swapped_differ']} of {dense.size} dots differ in bits from the swapped pair's")
    assert out["dense_differ"] >= 192 and out["swapped_differ"] >= 96
    found = so.one_ulp_pairs()
    print(f"{len(found)} of 300 one-ulp pairs have a negative squared distance before the clamp")
    if not found:
        sys.exit("no pair with a negative squared distance was found: the fixture cannot pin the clamp")
    a, b, sq = found[0]
    _, ra, _, ca = so.pack([a])
    out.update({"neg_count": len(found), "neg_ranks": ra, "neg_cores_a": ca, "neg_cores_b": so.pack([b])[3], "neg_sq": np.asarray(sq, dtype=F)})
    path = os.path.join(HERE, "tt_similarity_small.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
