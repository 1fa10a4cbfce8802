#!/usr/bin/env python3
"""Writes tests/golden/hnsw_mixed_small.npz from tests/_hnsw_mixed_oracle.py ALONE (never from the library): golden_corpus() —
400 x 20, every second row inserted Sparse with 70 % of its elements zeroed — built under DotProduct and under Cosine with the
default config; per metric the graph (levels, lists, entry point, maximum layer), the answers to 64 dense queries and to their
from_dense() sparse forms (k 10, ef 50), the answers of an ALL-DENSE oracle index over the to_dense() rows to the dense queries, and
the number of queries whose ids or score bits differ between the two.

    python tests/golden/make_golden_hnsw_mixed.py
"""
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests import _hnsw_mixed_oracle as mo  # noqa: E402
from tests import _hnsw_oracle as ho  # noqa: E402


def main():
    rows, mask, queries = mo.golden_corpus()
    out = {"rows": rows, "sparse_mask": mask, "queries": queries}
    sqs = [mo.SparseVector.from_dense(q) for q in queries]
    t = time.time()
    for name, metric in (("dot", ho.DOT_PRODUCT), ("cosine", ho.COSINE)):
        idx = mo.build_mixed(rows, mask, ho.HNSWConfig().with_distance_metric(metric))
        dense = ho.build(idx.to_dense_rows(), ho.HNSWConfig().with_distance_metric(metric))
        l0, l0cnt, up_head, up_ids = ho.golden_lists(idx)
        ids, sc, cnt = mo.answers_dense(idx, queries, 10, 50)
        sids, ssc, scnt = mo.answers_sparse(idx, sqs, 10, 50)
        dids, dsc, _ = ho.padded_answers(dense, queries, 10, 50)
        differ = int(((ids != dids) | (sc.view(np.uint32) != dsc.view(np.uint32))).any(axis=1).sum())
        print(f"{name}: {differ} of {len(queries)} queries differ from the all-dense index; max layer {idx.max_layer}, entry {idx.entry_point}")
        out.update({f"{name}_levels": np.asarray(idx.levels, dtype=np.int32), f"{name}_entry_point": idx.entry_point,
                    f"{name}_max_layer": idx.max_layer, f"{name}_l0": l0, f"{name}_l0cnt": l0cnt, f"{name}_up_head": up_head,
                    f"{name}_up_ids": up_ids, f"{name}_ids": ids, f"{name}_scores": sc, f"{name}_counts": cnt,
                    f"{name}_sparse_ids": sids, f"{name}_sparse_scores": ssc, f"{name}_sparse_counts": scnt,
                    f"{name}_dense_ids": dids, f"{name}_dense_scores": dsc, f"{name}_differ": differ})
    out["levels"] = out["dot_levels"]
    path = os.path.join(HERE, "hnsw_mixed_small.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {os.path.getsize(path)} bytes, oracle builds {time.time() - t:.1f} s")


if __name__ == "__main__":
    main()
