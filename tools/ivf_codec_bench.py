#!/usr/bin/env python
"""IVF-Flat / IVF-PQ / IVF-Binary on one MI355X, one synthetic corpus (neumann_amd/csrc/nmn_ivf.hip, nmn_ivf_codec.hip).

  python tools/ivf_codec_bench.py [--rows 2000000] [--dim 768] [--clusters 256] [--only flat,pq8,pq32,binary]

Every index trains on the first --train-rows rows (the exact GPU k-means; PQ also its per-subspace codebooks), gets the rest
through `add`, and then reports, for nprobe 8 and 16 at k = 10: the latency of a one-query call (median of --calls), the cost
per query of 64-query calls, and the device memory the index holds (nmn_ivf_hbm_bytes).  One JSON line per index."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

KINDS = {"flat": None, "pq8": 8, "pq32": 32, "binary": "sign"}


def build(kind, rows, clusters, capacity, args):
    from neumann_amd.ivf import GpuIvfBinary, GpuIvfFlat, GpuIvfPQ
    km = dict(max_iterations=args.train_iterations, seed=42, init_method="kmeans++", capacity_rows=capacity)
    if kind == "flat":
        return GpuIvfFlat.build(rows, clusters, **km)
    if kind.startswith("pq"):
        pq_km = dict(max_iterations=args.pq_iterations, seed=42, init_method="kmeans++")
        return GpuIvfPQ.build(rows, clusters, num_subspaces=KINDS[kind], num_centroids=256, pq_kmeans=pq_km, **km)
    return GpuIvfBinary.build(rows, clusters, threshold="sign", **km)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=2_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--clusters", type=int, default=256)
    ap.add_argument("--train-rows", type=int, default=100_000)
    ap.add_argument("--train-iterations", type=int, default=3)
    ap.add_argument("--pq-iterations", type=int, default=3)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--only", default="flat,pq8,pq32,binary")
    args = ap.parse_args()
    from neumann_amd.flat_index import synth_rows

    n, d = args.rows, args.dim
    tn = min(n, args.train_rows)
    Q1 = synth_rows(0x1F7, 0, args.calls, d)
    Q64 = synth_rows(0x1F8, 0, 64, d)
    for kind in args.only.split(","):
        t0 = time.perf_counter()
        ivf = build(kind, synth_rows(0x1F6, 0, tn, d), args.clusters, n, args)
        t_build = time.perf_counter() - t0
        out = {"index": kind, "rows": n, "dim": d, "clusters": args.clusters, "k": args.k, "train_rows": tn,
               "build_s": round(t_build, 2)}
        with ivf:
            t0 = time.perf_counter()
            for r0 in range(tn, n, 250_000):
                ivf.add(synth_rows(0x1F6, r0, min(250_000, n - r0), d))
            out["add_rows_per_s"] = round((n - tn) / (time.perf_counter() - t0)) if n > tn else None
            out["hbm_bytes"] = int(ivf._lib.nmn_ivf_hbm_bytes(ivf._h))
            for nprobe in (8, 16):
                ivf.search(Q1[0], args.k, nprobe)
                ivf.search(Q64, args.k, nprobe)
                lat = []
                for q in Q1:
                    t0 = time.perf_counter()
                    ivf.search(q, args.k, nprobe)
                    lat.append(time.perf_counter() - t0)
                reps = 5
                t0 = time.perf_counter()
                for _ in range(reps):
                    ivf.search(Q64, args.k, nprobe)
                per_q = (time.perf_counter() - t0) / (reps * 64)
                out[f"nprobe{nprobe}"] = {"ms_per_call_nq1": round(float(np.median(lat)) * 1e3, 3),
                                          "ms_per_query_nq64": round(per_q * 1e3, 4)}
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
