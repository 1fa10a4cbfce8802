#!/usr/bin/env python3
"""Time the delta-vector family (docs/delta.md) on the device path and on the library's host path, on one handle per shape.

    python tools/delta_bench.py --rows 200000 --dim 128 --k 16 --keep 0.05 --out profiles/delta_bench_128.json
    python tools/delta_bench.py --rows 200000 --dim 768 --k 256 --keep 0.5 --host-rows 20000

Timed per shape: find_best (nmn_archetypes_find_best), encode_batch (nmn_archetypes_encode_batch), dot_dense
(nmn_delta_set_dot_dense, --nq queries, the set's mirror made before the clock starts) — host buffers in and out, so every time is
a call's wall time up to its last byte on the host, the copies included.  The host path runs --host-rows rows (its time grows
linearly in the rows: every row is an independent chain) and is reported per row.  Rows are archetype + noise at a few positions, so
that a threshold between the two noise levels keeps about --keep of the entries.  Before anything is timed the two paths' answers
are compared bit for bit on the host's rows; a difference ends the run.  Needs a GPU: without one the device path fails and so
does this tool.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from neumann_amd import ArchetypeRegistry  # noqa: E402
from neumann_amd import delta as nd  # noqa: E402


def make(rows, dim, k, keep, seed):
    rng = np.random.default_rng(seed)
    arch = rng.standard_normal((k, dim)).astype(np.float32)
    x = arch[rng.integers(0, k, size=rows)]
    x += (rng.standard_normal((rows, dim)) * 1e-4).astype(np.float32)
    big = rng.random((rows, dim)) < keep
    x += big * (rng.standard_normal((rows, dim)) * 0.1).astype(np.float32)
    return arch, x, 1e-2


def timed(fn, reps):
    fn()                                    # warm-up: code objects, first allocations
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append(time.perf_counter() - t0)
    return float(np.median(t)), float(min(t)), float(max(t))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=200000)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--k", type=int, default=16)
    ap.add_argument("--keep", type=float, default=0.05)
    ap.add_argument("--nq", type=int, default=8)
    ap.add_argument("--host-rows", type=int, default=20000)
    ap.add_argument("--small-rows", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    arch, x, threshold = make(a.rows, a.dim, a.k, a.keep, a.seed)
    q = np.random.default_rng(a.seed + 1).standard_normal((a.nq, a.dim)).astype(np.float32)
    reg = ArchetypeRegistry(a.dim, a.k)
    reg.register_batch(arch)
    hx = x[:min(a.host_rows, a.rows)]
    res = dict(rows=a.rows, dim=a.dim, k=a.k, keep=a.keep, nq=a.nq, host_rows=int(hx.shape[0]), small_rows=a.small_rows, threshold=threshold,
               reps=a.reps)

    # the two paths on the host's rows: the same bits, or nothing below means anything
    reg.set_min_device_rows(nd.NEVER_DEVICE)
    h_ids, h_sims = reg.find_best_batch(hx)
    h_set = reg.encode_batch(hx, threshold, True)
    h_dot = h_set.dot_dense(q)
    reg.set_min_device_rows(nd.ALWAYS_DEVICE)
    d_ids, d_sims = reg.find_best_batch(hx)
    d_set = reg.encode_batch(hx, threshold, True)
    same = (np.array_equal(h_ids, d_ids) and np.array_equal(h_sims.view(np.uint32), d_sims.view(np.uint32))
            and np.array_equal(h_set.positions, d_set.positions) and np.array_equal(h_set.deltas.view(np.uint32), d_set.deltas.view(np.uint32))
            and np.array_equal(h_dot.view(np.uint32), d_set.dot_dense(q).view(np.uint32)))
    res["paths_agree_bit_for_bit"] = bool(same)
    if not same:
        print(json.dumps(res))
        return 1
    res["kept_fraction"] = float(d_set.nnz) / float(hx.size)

    for name, rows, mdr in (("device", x, nd.ALWAYS_DEVICE), ("device_small", x[:a.small_rows], nd.ALWAYS_DEVICE), ("host", hx, nd.NEVER_DEVICE)):
        reg.set_min_device_rows(mdr)
        n = rows.shape[0]
        s = reg.encode_batch(rows, threshold, True)
        if name != "host":
            s.to_device()
        for op, fn in (("find_best", lambda: reg.find_best_batch(rows)), ("encode_batch", lambda: reg.encode_batch(rows, threshold, True)),
                       ("dot_dense", lambda: s.dot_dense(q))):
            med, lo, hi = timed(fn, a.reps)
            res[f"{name}_{op}_s"] = med
            res[f"{name}_{op}_min_max_s"] = [lo, hi]
            res[f"{name}_{op}_us_per_row"] = med / n * 1e6
    for op in ("find_best", "encode_batch", "dot_dense"):
        per_dev, per_host = res[f"device_{op}_us_per_row"], res[f"host_{op}_us_per_row"]
        res[f"{op}_host_over_device"] = per_host / per_dev
        # the rows the host path gets through in the time a device call of --small-rows rows takes: below it the host wins
        res[f"{op}_crossover_rows"] = int(res[f"device_small_{op}_s"] / (per_host * 1e-6))
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
