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


def search_bench(a, reg, x, q_all, threshold, res):
    """--search: DeltaSet.search (docs/delta.md §8) at k = --top-k over --rows rows, per --search-nq: the call with host buffers, the
    stream-ordered call on resident tensors (enqueue to synchronize), the score kernels alone on resident tensors, and the same
    search at k = select_max_k + 1, which takes the sort of the large-k path — the only way the score array could be ranked before
    the select kernel.  First the host path and the device path are compared bit for bit on --host-rows rows."""
    import torch
    max_k = nd.search_limits()[1]
    hx = x[:min(a.host_rows, a.rows)]
    reg.set_min_device_rows(nd.NEVER_DEVICE)
    h_set = reg.encode_batch(hx, threshold, True)
    host_answers = [h_set.search(q_all[:8], k, m) for k in (a.top_k, max_k + 1) for m in ("dot", "cosine")]
    res["host_search_s"] = timed(lambda: h_set.search(q_all[:8], a.top_k), a.reps)[0]
    reg.set_min_device_rows(nd.ALWAYS_DEVICE)
    d_set = reg.encode_batch(hx, threshold, True)
    dev_answers = [d_set.search(q_all[:8], k, m) for k in (a.top_k, max_k + 1) for m in ("dot", "cosine")]
    same = all(np.array_equal(h[0], d[0]) and np.array_equal(h[1].view(np.uint32), d[1].view(np.uint32)) and np.array_equal(h[2], d[2])
               for h, d in zip(host_answers, dev_answers))
    res["paths_agree_bit_for_bit"] = bool(same)
    if not same:
        return 1
    s = reg.encode_batch(x, threshold, True).to_device()
    n = len(s)
    res["search_top_k"], res["large_k"] = a.top_k, max_k + 1

    def resident(fn):
        def run():
            fn()
            torch.cuda.synchronize()
        return run
    for nq in a.search_nq:
        q = q_all[:nq]
        tq = torch.from_numpy(q).cuda()
        scratch = torch.empty(s.search_scratch_bytes(nq, max_k + 1), dtype=torch.uint8, device="cuda")
        fscratch = torch.empty(s.scratch_floats(nq), dtype=torch.float32, device="cuda")
        out = torch.empty((nq, n), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        for name, fn in (("host_buffers", lambda: s.search(q, a.top_k)),
                         ("resident", resident(lambda: s.search_device(tq, a.top_k, scratch=scratch))),
                         ("resident_scores_only", resident(lambda: s.dot_dense_device(tq, out=out, scratch=fscratch))),
                         ("resident_large_k_path", resident(lambda: s.search_device(tq, max_k + 1, scratch=scratch)))):
            med, lo, hi = timed(fn, a.reps)
            res[f"search_nq{nq}_{name}_s"] = med
            res[f"search_nq{nq}_{name}_min_max_s"] = [lo, hi]
        res[f"search_nq{nq}_select_bytes_read"] = 4 * n * 4 * nq          # the yardstick: 4 passes x n x 4 bytes per query
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--search", action="store_true", help="time DeltaSet.search instead of find_best / encode_batch / dot_dense")
    ap.add_argument("--top-k", type=int, default=10)
    ap.add_argument("--search-nq", type=int, nargs="+", default=[1, 8, 64])
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
    if a.search:
        q_all = np.random.default_rng(a.seed + 1).standard_normal((max(a.search_nq + [8]), a.dim)).astype(np.float32)
        rc = search_bench(a, reg, x, q_all, threshold, res)
        line = json.dumps(res)
        print(line)
        if a.out and rc == 0:
            with open(a.out, "w") as f:
                f.write(line + "\n")
        return rc

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
    # a set made where the rows are (docs/delta.md §9): the rows resident, the call up to a device synchronize; and, apart, the first
    # arrays() of such a set — the download the host-buffer encode_batch used to include
    import torch
    reg.set_min_device_rows(nd.ALWAYS_DEVICE)
    reg.to_device()
    tx = torch.from_numpy(x).cuda()
    torch.cuda.synchronize()

    def born():
        s = reg.encode_batch_device(tx, threshold, True)
        torch.cuda.synchronize()
        return s
    med, lo, hi = timed(born, a.reps)
    res["device_encode_batch_device_s"], res["device_encode_batch_device_min_max_s"] = med, [lo, hi]
    first = []
    for _ in range(a.reps):
        s = born()
        t0 = time.perf_counter()
        s.arrays()
        first.append(time.perf_counter() - t0)
    res["device_first_arrays_s"], res["device_first_arrays_min_max_s"] = float(np.median(first)), [float(min(first)), float(max(first))]
    h = reg.encode_batch(x[:a.host_rows], threshold, True)
    d = reg.encode_batch_device(tx[:a.host_rows], threshold, True)
    res["device_born_equals_host_buffer_set"] = bool(all(np.array_equal(h.arrays()[k].view(np.uint8), d.arrays()[k].view(np.uint8)) for k in h.arrays()))
    # the whole batch through the host-buffer call (above 256 MiB of rows: several chunks, joined on the device) against the same
    # rows encoded where they are
    full_h, full_d = reg.encode_batch(x, threshold, True).arrays(), born().arrays()
    res["chunked_equals_device_born"] = bool(all(np.array_equal(full_h[k].view(np.uint8), full_d[k].view(np.uint8)) for k in full_h))
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
