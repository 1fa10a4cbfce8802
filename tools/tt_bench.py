#!/usr/bin/env python3
"""Measure nmn_tt_decompose (docs/hnsw.md §21): the device kernel by HIP events against the host restatement on 1 and 16 threads
(the CPU form of the reference's rayon batch), on 100 000 x 768 and 20 000 x 4096 vectors under TTConfig::for_dim, per workgroup
size (64, 128, 256 threads own a vector), and at batch sizes 1 .. 4096 for the crossover behind NMN_TT_DECOMPOSE_MIN.

    python tools/tt_bench.py --out profiles/tt_decompose_bench.jsonl        # every configuration, each in its own process
    python tools/tt_bench.py --child device --dim 768 --n 100000 --threads 64

Every configuration runs as its own process under its own time limit; a child prints one JSON line.  Times are medians of
--reps runs after a warm-up run; the device time is the kernel alone (events on the stream around the enqueue, the vectors
already resident), the host time is the whole host call."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def vectors(n, dim):
    import numpy as np
    return np.random.default_rng(dim * 1000003 + n).standard_normal((n, dim)).astype(np.float32)


def child_device(a):
    import ctypes as C
    import numpy as np
    import torch
    from neumann_amd import TTConfig, _capi, tt
    os.environ["NMN_TT_DECOMPOSE_THREADS"] = str(a.threads)
    if a.grid:
        os.environ["NMN_TT_DECOMPOSE_GRID"] = str(a.grid)
    lib = _capi.load()
    cfg = TTConfig.for_dim(a.dim)
    sh = np.asarray(cfg.shape, dtype=np.uint32)
    slot = cfg.max_storage
    vt = torch.from_numpy(vectors(a.n, a.dim)).cuda()
    status = torch.zeros(a.n, dtype=torch.int32, device="cuda")
    ranks = torch.zeros((a.n, sh.size + 1), dtype=torch.int32, device="cuda")
    cores = torch.zeros(a.n * slot, dtype=torch.float32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream

    def run():
        _capi.check(lib.nmn_tt_decompose_device(C.c_void_p(vt.data_ptr()), a.n, a.dim, C.c_void_p(sh.ctypes.data), sh.size, cfg.max_rank,
                                                C.c_float(cfg.tolerance), C.c_void_p(status.data_ptr()), C.c_void_p(ranks.data_ptr()), None,
                                                C.c_void_p(cores.data_ptr()), cores.numel(), C.c_void_p(stream)))
    run()
    torch.cuda.synchronize()
    ms = []
    for _ in range(a.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        run()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    med = statistics.median(ms)
    print(json.dumps({"kind": "device_kernel", "dim": a.dim, "shape": cfg.shape, "max_rank": cfg.max_rank, "n": a.n,
                      "threads_per_vector": a.threads, "grid": a.grid or "default", "lds_floats": tt.decompose_lds_floats(cfg),
                      "ms_median": med, "ms_all": ms, "vectors_per_s": a.n / (med * 1e-3), "ok": int((status == 0).sum().item())}))


def child_call(a):
    """the whole host-buffer call, nmn_tt_decompose: on the host restatement (--host-threads) or on the device (upload, kernel,
    read-back and packing included)"""
    import numpy as np
    from neumann_amd import TTConfig, tt
    if a.host_threads:
        os.environ["NMN_HNSW_HOST_SEARCH"] = "1"
        os.environ["NMN_TT_DECOMPOSE_HOST_THREADS"] = str(a.host_threads)
    else:
        os.environ["NMN_TT_DECOMPOSE_MIN"] = "0"
    cfg = TTConfig.for_dim(a.dim)
    v = vectors(a.n, a.dim)
    tt.tt_decompose_raw(v[:max(1, min(a.n, 64))], cfg)
    ms = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        tt.tt_decompose_raw(v, cfg)
        ms.append((time.perf_counter() - t0) * 1e3)
    med = statistics.median(ms)
    print(json.dumps({"kind": f"host_{a.host_threads}_threads" if a.host_threads else "device_call", "dim": a.dim, "n": a.n,
                      "ms_median": med, "ms_all": ms, "vectors_per_s": a.n / (med * 1e-3)}))


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--child", choices=["device", "call"])
    p.add_argument("--dim", type=int, default=768)
    p.add_argument("--n", type=int, default=100000)
    p.add_argument("--threads", type=int, default=64)
    p.add_argument("--grid", type=int, default=0)
    p.add_argument("--host-threads", type=int, default=0)
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--out", default=None)
    p.add_argument("--limit", type=int, default=120, help="seconds per configuration")
    p.add_argument("--quick", action="store_true", help="a tenth of the vectors")
    a = p.parse_args()
    if a.child:
        return child_device(a) if a.child == "device" else child_call(a)
    scale = 10 if a.quick else 1
    jobs = []
    for dim, n in ((768, 100000 // scale), (4096, 20000 // scale)):
        for threads in (64, 128, 256):
            jobs.append(["--child", "device", "--dim", dim, "--n", n, "--threads", threads])
        jobs.append(["--child", "call", "--dim", dim, "--n", n // 50, "--host-threads", 1, "--reps", 3])
        jobs.append(["--child", "call", "--dim", dim, "--n", n // 5, "--host-threads", 16, "--reps", 3])
    for grid in (512, 1024, 4096):
        jobs.append(["--child", "device", "--dim", 768, "--n", 100000 // scale, "--threads", 64, "--grid", grid])
    for n in (1, 2, 4, 8, 16, 32, 64, 128, 256, 1024, 4096):     # the crossover, (8,8,12) with rank 8
        jobs.append(["--child", "call", "--dim", 768, "--n", n, "--host-threads", 1 if n < 64 else 16, "--reps", 7])
        jobs.append(["--child", "call", "--dim", 768, "--n", n, "--reps", 7])
    lines = []
    for j in jobs:
        cmd = [sys.executable, os.path.abspath(__file__)] + [str(x) for x in j]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.limit)
        except subprocess.TimeoutExpired:
            print(json.dumps({"args": j, "error": "time limit"}), flush=True)
            return 1      # nothing more is started on the GPU after a step that did not end
        if r.returncode != 0:
            print(json.dumps({"args": j, "error": r.stderr[-400:], "code": r.returncode}), flush=True)
            return 1
        line = r.stdout.strip().splitlines()[-1]
        print(line, flush=True)
        lines.append(line)
        if a.out:
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
