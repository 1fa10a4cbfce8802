#!/usr/bin/env python3
"""Measure nmn_tt_decompose (docs/hnsw.md §21): the device kernel by HIP events against the host restatement on 1 and 16 threads
(the CPU form of the reference's rayon batch), on 100 000 x 768 and 20 000 x 4096 vectors under TTConfig::for_dim, per workgroup
size (64, 128, 256 threads own a vector), and at batch sizes 1 .. 4096 for the crossover behind NMN_TT_DECOMPOSE_MIN.

    python tools/tt_bench.py --out profiles/tt_decompose_bench.jsonl        # every configuration, each in its own process
    python tools/tt_bench.py --child device --dim 768 --n 100000 --threads 64
    python tools/tt_bench.py --similarity --out profiles/tt_similarity_bench.jsonl

--similarity measures nmn_tt_similarity (docs/hnsw.md §23) instead: trains of shape (8,8,12) at ranks [1,8,8,1], 1 x 100 000 and
64 x 100 000 pairs, the kernels alone by HIP events with the trains resident, the whole host-buffer call, the host restatement on 1
and 16 threads, and one query against 1 .. 16 384 targets for the crossover behind NMN_TT_SIMILARITY_MIN.

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


SIM_SHAPE, SIM_RANKS = (8, 8, 12), (1, 8, 8, 1)     # TTConfig::for_dim(768) at its full ranks: 672 core floats a train


def sim_sets(nq, nt):
    """-> (shape u32, stride, (ranks, core_off, cores) of the queries, the same of the targets): Gaussian cores scaled so that the
    dots stay near 1"""
    import numpy as np
    stride = sum(SIM_RANKS[k] * SIM_SHAPE[k] * SIM_RANKS[k + 1] for k in range(3))
    rng = np.random.default_rng(nq * 1000003 + nt)

    def one(n):
        ranks = np.tile(np.asarray(SIM_RANKS, dtype=np.uint32), (n, 1))
        off = np.arange(n + 1, dtype=np.uint64) * np.uint64(stride)
        return ranks, off, (rng.standard_normal(n * stride) * 0.35).astype(np.float32)
    return np.asarray(SIM_SHAPE, dtype=np.uint32), stride, one(nq), one(nt)


def child_sim_device(a):
    """the kernels alone by HIP events, the trains resident: the self-dot pass over the targets, then the similarity launch per op"""
    import numpy as np
    import torch
    from neumann_amd import tt
    shape, stride, q, t = sim_sets(a.nq, a.n)
    dev = lambda x: torch.from_numpy(x.view(np.int32) if x.dtype == np.uint32 else x).cuda()   # noqa: E731
    qs, ts = tt.TTDeviceSet(dev(q[0]), dev(q[2]), stride), tt.TTDeviceSet(dev(t[0]), dev(t[2]), stride)
    out = torch.empty((a.nq, a.n), dtype=torch.float32, device="cuda")
    self_q, self_t = tt.tt_self_dot_device(SIM_SHAPE, qs), tt.tt_self_dot_device(SIM_SHAPE, ts)

    def timed(fn):
        fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1))
        return statistics.median(ms), ms
    line = {"kind": "sim_device_kernel", "shape": SIM_SHAPE, "ranks": SIM_RANKS, "nq": a.nq, "nt": a.n, "pairs": a.nq * a.n}
    line["self_dot_ms_median"], line["self_dot_ms_all"] = timed(lambda: tt.tt_self_dot_device(SIM_SHAPE, ts, out=self_t))
    for op in ("dot", "cosine", "euclidean"):
        med, ms = timed(lambda: tt.tt_similarity_device(op, SIM_SHAPE, qs, ts, self_q, self_t, out=out))
        line[f"{op}_ms_median"], line[f"{op}_ms_all"] = med, ms
        line[f"{op}_pairs_per_s"] = a.nq * a.n / (med * 1e-3)
    line["finite"] = bool(torch.isfinite(out).all().item())
    print(json.dumps(line))


def child_sim_call(a):
    """the whole host-buffer call, nmn_tt_similarity (cosine: the self dots included): on the host restatement (--host-threads) or
    on the device (upload, three launches, read-back)"""
    import ctypes as C
    import numpy as np
    from neumann_amd import _capi
    if a.host_threads:
        os.environ["NMN_HNSW_HOST_SEARCH"] = "1"
        os.environ["NMN_TT_SIMILARITY_HOST_THREADS"] = str(a.host_threads)
    else:
        os.environ["NMN_TT_SIMILARITY_MIN"] = "0"
    lib = _capi.load()
    shape, _, q, t = sim_sets(a.nq, a.n)
    out = np.empty((a.nq, a.n), dtype=np.float32)
    p = lambda x: C.c_void_p(x.ctypes.data)   # noqa: E731

    def run(nt):
        _capi.check(lib.nmn_tt_similarity(1, p(shape), 3, p(q[0]), p(q[1]), p(q[2]), a.nq, p(shape), 3, p(t[0]), p(t[1]), p(t[2]), nt, p(out)))
    run(min(a.n, 64))
    ms = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        run(a.n)
        ms.append((time.perf_counter() - t0) * 1e3)
    med = statistics.median(ms)
    print(json.dumps({"kind": f"sim_host_{a.host_threads}_threads" if a.host_threads else "sim_device_call", "op": "cosine", "nq": a.nq,
                      "nt": a.n, "pairs": a.nq * a.n, "ms_median": med, "ms_all": ms, "pairs_per_s": a.nq * a.n / (med * 1e-3)}))


def similarity_jobs(scale):
    jobs = []
    for nq in (1, 64):
        jobs.append(["--child", "sim_device", "--nq", nq, "--n", 100000 // scale])
        jobs.append(["--child", "sim_call", "--nq", nq, "--n", 100000 // scale])
        jobs.append(["--child", "sim_call", "--nq", nq, "--n", 100000 // scale // (50 * nq), "--host-threads", 1, "--reps", 3])
        jobs.append(["--child", "sim_call", "--nq", nq, "--n", 100000 // scale // (5 * nq), "--host-threads", 16, "--reps", 3])
    for n in (1, 4, 8, 16, 32, 64, 256, 1024, 4096, 16384):   # the crossover behind NMN_TT_SIMILARITY_MIN, one query; the host as
        jobs.append(["--child", "sim_call", "--nq", 1, "--n", n, "--host-threads", 16, "--reps", 7])   # the library routes it
        jobs.append(["--child", "sim_call", "--nq", 1, "--n", n, "--reps", 7])
    return jobs


def decompose_jobs(scale):
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
    return jobs


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--child", choices=["device", "call", "sim_device", "sim_call"])
    p.add_argument("--similarity", action="store_true", help="measure nmn_tt_similarity (docs/hnsw.md §23) instead of nmn_tt_decompose")
    p.add_argument("--nq", type=int, default=1)
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
        return {"device": child_device, "call": child_call, "sim_device": child_sim_device, "sim_call": child_sim_call}[a.child](a)
    scale = 10 if a.quick else 1
    jobs = similarity_jobs(scale) if a.similarity else decompose_jobs(scale)
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
