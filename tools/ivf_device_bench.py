#!/usr/bin/env python
"""The stream-ordered IVF search (nmn_ivf_search_device) against the host call (nmn_ivf_search) on one MI355X, one synthetic
corpus, IVF-Flat / IVF-PQ (M = 8) / IVF-Binary (docs/ivf.md §3.10c).

  python tools/ivf_device_bench.py [--rows 2000000] [--dim 768] [--clusters 256] [--only flat,pq8,binary]
  python tools/ivf_device_bench.py --launch-calls N ...   # N device calls per index and nothing else (for a kernel trace)

Every index trains on the first --train-rows rows and gets the rest through `add` (as tools/ivf_codec_bench.py).  For nprobe
8 and 16 at k = 10 it reports, per index:
  dev_ms_nq1 / dev_ms_nq64     device time of one call (HIP events around it on its stream; median of --calls)
  dev_ms_per_query_nq64        the same per query
  b2b_ms_per_call_nq1 / _nq64  200 calls back to back on one stream, one synchronise at the end (wall time / calls)
  host_ms_nq1 / host_ms_per_query_nq64  the host call nmn_ivf_search on the same index (wall time)
and checks that the device answers equal the host call's.  One JSON line per index.  Launches per call come from two runs of
--launch-calls under `rocprofv3 --kernel-trace --stats` (0 and N calls): the difference of the dispatch counts over N."""
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
    ap.add_argument("--b2b", type=int, default=200)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--only", default="flat,pq8,binary")
    ap.add_argument("--launch-calls", type=int, default=None)
    args = ap.parse_args()
    import torch
    from neumann_amd.flat_index import synth_rows

    n, d, k = args.rows, args.dim, args.k
    tn = min(n, args.train_rows)
    Q1 = synth_rows(0x1F7, 0, args.calls, d)
    Q64 = synth_rows(0x1F8, 0, 64, d)
    q1_t = [torch.from_numpy(Q1[i:i + 1].copy()).cuda() for i in range(args.calls)]
    q64_t = torch.from_numpy(Q64).cuda()
    s = torch.cuda.Stream()
    for kind in args.only.split(","):
        t0 = time.perf_counter()
        ivf = build(kind, synth_rows(0x1F6, 0, tn, d), args.clusters, n, args)
        out = {"index": kind, "rows": n, "dim": d, "clusters": args.clusters, "k": k, "build_s": round(time.perf_counter() - t0, 2)}
        with ivf:
            for r0 in range(tn, n, 250_000):
                ivf.add(synth_rows(0x1F6, r0, min(250_000, n - r0), d))
            torch.cuda.synchronize()
            if args.launch_calls is not None:
                with torch.cuda.stream(s):
                    for i in range(args.launch_calls):
                        ivf.search_device(q1_t[i % args.calls], k, 8)
                s.synchronize()
                out["device_calls"] = args.launch_calls
                print(json.dumps(out), flush=True)
                continue
            out["hbm_bytes_before_device_search"] = ivf.hbm_bytes
            for nprobe in (8, 16):
                r = {}
                with torch.cuda.stream(s):
                    out1 = (torch.empty((1, k), dtype=torch.int64, device="cuda"), torch.empty((1, k), dtype=torch.float32, device="cuda"),
                            torch.empty((1,), dtype=torch.int32, device="cuda"))
                    out64 = (torch.empty((64, k), dtype=torch.int64, device="cuda"), torch.empty((64, k), dtype=torch.float32, device="cuda"),
                             torch.empty((64,), dtype=torch.int32, device="cuda"))
                    # warm-up (workspace, id map) and the answers against the host call's
                    got1 = ivf.search_device(q1_t[0], k, nprobe, out=out1)
                    got64 = ivf.search_device(q64_t, k, nprobe, out=out64)
                    s.synchronize()
                    w1, w64 = ivf.search(Q1[0], k, nprobe), ivf.search(Q64, k, nprobe)
                    same = all(np.array_equal(g[0].cpu().numpy().view(np.uint64), w[0]) and
                               np.array_equal(g[1].cpu().numpy().view(np.uint32), w[1].view(np.uint32)) and
                               np.array_equal(g[2].cpu().numpy().astype(np.uint32), w[2]) for g, w in ((got1, w1), (got64, w64)))
                    r["device_equals_host_call"] = bool(same)
                    for name, qs, o in (("nq1", q1_t, out1), ("nq64", [q64_t] * args.calls, out64)):
                        ts = []
                        for q in qs:
                            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                            e0.record(s)
                            ivf.search_device(q, k, nprobe, out=o)
                            e1.record(s)
                            ts.append((e0, e1))
                        s.synchronize()
                        r[f"dev_ms_{name}"] = round(float(np.median([a.elapsed_time(b) for a, b in ts])), 4)
                        s.synchronize()
                        t0 = time.perf_counter()
                        for i in range(args.b2b):
                            ivf.search_device(qs[i % len(qs)], k, nprobe, out=o)
                        s.synchronize()
                        r[f"b2b_ms_per_call_{name}"] = round((time.perf_counter() - t0) * 1e3 / args.b2b, 4)
                r["dev_ms_per_query_nq64"] = round(r["dev_ms_nq64"] / 64, 4)
                r["b2b_ms_per_query_nq64"] = round(r["b2b_ms_per_call_nq64"] / 64, 4)
                lat = []
                for q in Q1:
                    t0 = time.perf_counter()
                    ivf.search(q, k, nprobe)
                    lat.append(time.perf_counter() - t0)
                r["host_ms_nq1"] = round(float(np.median(lat)) * 1e3, 4)
                t0 = time.perf_counter()
                for _ in range(5):
                    ivf.search(Q64, k, nprobe)
                r["host_ms_per_query_nq64"] = round((time.perf_counter() - t0) * 1e3 / (5 * 64), 4)
                out[f"nprobe{nprobe}"] = r
            out["hbm_bytes_after_device_search"] = ivf.hbm_bytes
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
