#!/usr/bin/env python3
"""Writes tests/golden/hnsw_ttnode_small.npz from tests/_hnsw_ttnode_oracle.py ALONE (never from the library): 400 trains of shape
[2,2,5], ranks [1,2,2,1] (golden_sets()), every second one inserted as a TensorTrain node and the others as Dense(reconstruction),
one train in eight scaled so that the cached norms straddle 1e-10; built under Cosine, Euclidean and DotProduct with the default
config.  Per metric: the graph (levels, every neighbour list, the entry point), the answers to 64 dense queries and to 64 TT queries
at k 10, ef 50, and — against the index of the SAME rows inserted as Dense(reconstruction) nodes, what insert_tt_vector makes — the
number of nodes whose neighbour lists differ, of dense-query answers that differ, of TT-query answers that differ and of TT-query
answers whose ids differ.  The script fails unless the fixture tells the two kinds of node apart (docs/hnsw.md §24).

    python tests/golden/make_golden_hnsw_ttnode.py
"""
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests import _hnsw_mixed_oracle as mo  # noqa: E402
from tests import _hnsw_oracle as ho  # noqa: E402
from tests import _hnsw_tt_oracle as to  # noqa: E402
from tests import _hnsw_ttnode_oracle as tn  # noqa: E402

F = np.float32


def main():
    trains, tt_mask, dense_q, tt_q = tn.golden_sets()
    shape, ranks, off, cores = to.pack(trains)
    qshape, qranks, qoff, qcores = to.pack(tt_q)
    norms = np.asarray([to.tt_norm(t) for t in trains], dtype=F)
    recon = np.stack([to.tt_reconstruct(t) for t in trains])
    mags = np.asarray([ho.magnitude(r) for r in recon], dtype=F)
    node_norms = norms[tt_mask]
    below, near = int((node_norms < tn.TINY).sum()), int(((node_norms >= tn.TINY) & (node_norms < F(1e-8))).sum())
    print(f"{below} TT-node norms below 1e-10, {near} in [1e-10, 1e-8); {int((norms.view(np.uint32) != mags.view(np.uint32)).sum())} "
          f"of {len(trains)} norms differ in bits from simd::magnitude of the reconstruction")
    assert below >= 4 and near >= 4, (below, near)
    out = {"shape": shape, "ranks": ranks, "core_off": off, "cores": cores, "tt_mask": tt_mask, "norms": norms,
           "reconstructions": recon, "dense_queries": dense_q, "q_ranks": qranks, "q_core_off": qoff, "q_cores": qcores,
           "norms_below": below, "norms_near": near}
    t = time.time()
    for name, metric in (("cosine", ho.COSINE), ("euclidean", ho.EUCLIDEAN), ("dot", ho.DOT_PRODUCT)):
        idx = tn.golden_index(trains, tt_mask, metric)
        twin = tn.golden_index(trains, tt_mask, metric, as_dense=True)
        assert idx.levels == twin.levels
        l0, l0cnt, up_head, up_ids = ho.golden_lists(idx)
        d = mo.answers_dense(idx, dense_q, 10, 50)
        q = tn.answers_tt(idx, tt_q, 10, 50)
        dd = mo.answers_dense(twin, dense_q, 10, 50)
        qd = tn.answers_tt(twin, tt_q, 10, 50)
        counts = {"lists_differ": tn.lists_differ(idx, twin), "dense_differ": tn.answers_differ(d, dd),
                  "tt_differ": tn.answers_differ(q, qd), "tt_ids_differ": int((q[0] != qd[0]).any(axis=1).sum())}
        print(name, counts)
        if metric == ho.COSINE:
            assert counts["lists_differ"] >= 1 and counts["dense_differ"] >= 32, counts
        assert counts["tt_differ"] >= 32, counts
        out.update({f"{name}_levels": np.asarray(idx.levels, dtype=np.int32), f"{name}_entry_point": idx.entry_point,
                    f"{name}_max_layer": idx.max_layer, f"{name}_l0": l0, f"{name}_l0cnt": l0cnt, f"{name}_up_head": up_head,
                    f"{name}_up_ids": up_ids, f"{name}_ids": d[0], f"{name}_scores": d[1], f"{name}_counts": d[2],
                    f"{name}_tt_ids": q[0], f"{name}_tt_scores": q[1], f"{name}_tt_counts": q[2]})
        out.update({f"{name}_{k}": v for k, v in counts.items()})
    path = os.path.join(HERE, "hnsw_ttnode_small.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {os.path.getsize(path)} bytes, oracle builds {time.time() - t:.1f} s")


if __name__ == "__main__":
    main()
