#!/usr/bin/env python3
"""Write tests/golden/delta_small.npz: a small mixed case of delta vectors with the outputs of the twin tests/_delta_oracle.py, and
the inputs of the reference's own unit tests (tensor_store/src/delta_vector.rs, mod tests: test_delta_reconstruction,
test_delta_dot_dense) with the twin's exact answers, restated as data.

    python -m tests.golden.make_golden_delta          # rewrite the fixture
    python -m tests.golden.make_golden_delta --check  # exit 1 if the committed file is not what this script computes

The script counts how many of the fixture's dot products differ in bits from two naive formulations and refuses to write a fixture
that cannot tell them apart:
  pairwise_differ   against NumPy's own f32 `sum` of the products of the decoded row and the query (pairwise, unrolled);
  plus_zero_differ  against the same sequential chains folded from +0.0 instead of -0.0: the -0.0 answers, which a fold from +0.0
                    can never give.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from tests import _delta_oracle as do  # noqa: E402

F = np.float32
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "delta_small.npz")
DIM, K, N, NQ, THRESHOLD = 48, 5, 40, 3, 0.05


def inputs():
    rng = np.random.default_rng(20260)
    arch = rng.standard_normal((K, DIM)).astype(F)
    arch[3] = 0.0                                     # a zero archetype
    rows = np.empty((N, DIM), dtype=F)
    for i in range(N):
        rows[i] = arch[i % K] + (rng.standard_normal(DIM) * (0.2 if i % 3 else 0.02)).astype(F)
    rows[3] = 0.0                                     # a zero row: archetype 0, similarity 0.0, every entry kept or none
    for i in (8, 23):                                 # small rows against every other archetype: the zero archetype wins with 0.0, no
        rows[i] = F(-0.004 * (1 + i % 2)) * (arch[0] + arch[1] + arch[2] + arch[4])   # entry is kept, and its dot with q[0] is -0.0
    rows[11] = arch[1]                                # equal to its archetype: no entries
    q = rng.standard_normal((NQ, DIM)).astype(F)
    q[0] = -np.abs(q[0]) - F(0.25)                    # all negative: the zero archetype's dot is -0.0
    return arch, rows, q


def compute():
    arch, rows, q = inputs()
    reg = do.ArchetypeRegistry(K)
    for a in arch:
        reg.register(a)
    ids, sims = reg.find_best_many(rows)
    cached = [d for d, _ in reg.encode_batch(rows, THRESHOLD, True)]
    plain = [d for d, _ in reg.encode_batch(rows, THRESHOLD, False)]
    p = do.pack(cached)
    dot = do.dot_dense_all(reg, cached, q)
    decoded = do.decode_all(reg, cached)
    pairs = np.asarray([(i, (i + K) % N) for i in range(N)] + [(0, 1), (2, 3), (5, 5)], dtype=np.uint64)
    pair_dot, pair_ok = do.pairs_all(reg, cached, cached, pairs)
    naive = np.stack([(decoded * qq[None, :]).sum(axis=1, dtype=F) for qq in q])
    minus_zero = do.bits_of(dot) == 0x80000000
    out = dict(archetypes=arch, rows=rows, queries=q, threshold=F(THRESHOLD), best_ids=ids.astype(np.int64), best_sims=sims,
               magnitude_sq=np.asarray(reg.magnitude_sq_, dtype=F), indptr=p["indptr"], positions=p["positions"], deltas=p["deltas"],
               cached=p["cached_magnitudes"], dot=dot, cosine=do.cosine_dense_all(reg, cached, q), decoded=decoded,
               magnitudes_uncached=do.magnitudes(reg, plain), pairs=pairs, pair_ok=pair_ok, pair_dot=pair_dot,
               pairwise_differ=np.int64((do.bits_of(dot) != do.bits_of(naive)).sum()), plus_zero_differ=np.int64(minus_zero.sum()))
    # the reference's unit tests as data: archetype, vector, threshold 0.001, query
    ka, kv, kq = np.asarray([1.0, 0.0, 0.0, 0.0], dtype=F), np.asarray([0.9, 0.1, 0.05, 0.0], dtype=F), np.asarray([1.0, 1.0, 0.0, 0.0], dtype=F)
    kd = do.DeltaVector.from_dense_with_reference(kv, ka, 0, 0.001)
    out.update(kat_archetype=ka, kat_dense=kv, kat_query=kq, kat_positions=kd.positions, kat_deltas=kd.deltas,
               kat_reconstructed=kd.to_dense(ka), kat_dot=np.asarray(kd.dot_dense(kq, ka), dtype=F))
    return out


def main():
    out = compute()
    assert out["pairwise_differ"] > 0 and out["plus_zero_differ"] > 0, "the fixture cannot tell the naive sums apart: choose other inputs"
    if "--check" in sys.argv:
        z = np.load(OUT)
        ok = sorted(z.files) == sorted(out) and all(z[k].tobytes() == np.asarray(out[k]).tobytes() for k in z.files)
        print("current" if ok else "stale")
        return 0 if ok else 1
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), "bytes; pairwise_differ", int(out["pairwise_differ"]), "of", out["dot"].size, "plus_zero_differ",
          int(out["plus_zero_differ"]))
    return 0


if __name__ == "__main__":
    sys.exit(main())
