#!/usr/bin/env python
"""The GPU graph walk (nmn_hnsw_search / nmn_hnsw_search_device) against the exhaustive search over the same rows
(nmn_index_search through nmn_hnsw_vectors) and against the host walk (NMN_HNSW_HOST_SEARCH=1), on one MI355X and one
synthetic corpus (docs/hnsw.md §6).

  timeout -k 10 1100 python tools/hnsw_bench.py --rows 1000000 --dim 128 && \\
  timeout -k 10 1100 python tools/hnsw_bench.py --rows 200000 --dim 768
  python tools/hnsw_bench.py --launch-calls N ...   # N device calls and nothing else (for `rocprofv3 --kernel-trace --stats -- ...`)

(each corpus a process of its own under its own time limit, chained: a failure ends the chain).  The graph is built on the host
by nmn_hnsw_insert — one thread, the reference's sequential algorithm — and `build_s` says how long that took.  For ef_search 50
and 200 at k = 10 it reports, as one JSON line:
  gpu_ms_nq1                  a lone nmn_hnsw_search call, host buffers (wall time, median of --calls)
  gpu_ms_per_query_nq64/1024  the same call with 64 / 1024 queries, per query
  dev_ms_per_query_nq64/1024  nmn_hnsw_search_device, HIP events around the call on its stream (median of --calls), per query
  b2b_ms_per_query_nq64       --b2b device calls back to back on one stream, one synchronise at the end
  flat_ms_nq1 / flat_ms_per_query_nq64/1024   nmn_index_search over the same rows, measured ALTERNATING with the walk
  host_ms_per_query           the host walk, wall time per query over 64 queries
  *_spread                    (max - min) / median over --repeats repetitions of the whole measurement
  recall_at_10                of the walk against the exhaustive search (1024 queries)
  evals_per_query             distance evaluations per query (nmn_search_stats.rows_scanned)
and checks that device, host-buffer and host-walk answers are the same bits.

  python tools/hnsw_bench.py --rows 50000 --dim 128 --metric composite     # or cosine, angular, weighted_jaccard, ...
With a NAME instead of a number, --metric is an ExtendedDistanceMetric and the tool times the re-rank instead (docs/hnsw.md §8):
nmn_hnsw_search_metric_device at top_k = --k beside nmn_hnsw_search_device at k = c = max(2 top_k, 10) — the walk alone, the same
candidates — at the preset's ef_search (50 by default), 1 / 64 / 1024 queries per call, HIP events around each call on one stream, the two alternating call by
call: medians of --calls (a fifth of it at 1024 queries), spread over --repeats repetitions.  The index metric stays cosine.
--launch-calls N then makes N search_metric_device calls and nothing else.

  python tools/hnsw_bench.py --rows 200000 --dim 768 --storage quantized
  python tools/hnsw_bench.py --rows 200000 --dim 128 --storage binary [--binary-threshold sign|mean|median]
builds the corpus twice — a quantized handle (HNSWStorageStrategy::Quantized, docs/hnsw.md §9) and a dense one — and times the
quantized walk beside the dense walk OF THE SAME RUN, the two alternating call by call: nmn_hnsw_search_device under HIP events at
1 / 64 / 1024 queries per call and a lone host-buffer nmn_hnsw_search call, ef 50 and 200, medians of --calls, spread over
--repeats.  It prints both handles' hbm_bytes, build times, evaluations per query and recall@10 of each against the exhaustive
search over the f32 rows, and checks that the quantized handle's device, host-buffer and host-walk answers are the same bits.
With --storage binary the binary handle (EmbeddingStorage::Binary nodes, docs/hnsw.md §18) stands in the quantized one's place and
the keys say "bin"; it has no file form and is built every run, --index-file then names the DENSE handle's file.

  python tools/hnsw_bench.py --rows 1000000 --dim 128 --index-file /data/hnsw_1m_128.idx
With --index-file the run stops paying for builds (docs/hnsw.md §10): when PATH exists the handle is GpuHnsw.load(PATH) and the
output has load_s and index_file_bytes; otherwise the corpus is built as before, saved to PATH and loaded back once, and the
output has build_s, save_s, load_s and index_file_bytes.  The file must hold the index the other arguments describe (rows, dim,
preset, metric, storage) or the run ends.  With --storage quantized, PATH is the quantized handle's file and PATH + ".dense" the
dense one's.

  python tools/hnsw_bench.py --rows 1000000 --dim 128 --index-file PATH --callers 1,16,64,128 [--storage quantized]
--callers times CONCURRENT host callers and nothing else (docs/hnsw.md §11): for every N of the list, N threads behind a barrier,
each making --caller-calls calls of nmn_hnsw_search(nq = 1) with k taken in turn from 1, 10, 50, 100 (ef_search of the preset).
Per N it reports queries_per_s (all calls / wall time), call_ms_median (one call as its caller saw it), and what
nmn_hnsw_coalesce_stats counted meanwhile (merged batches, the calls in them, calls per merged batch); medians and spread over
--repeats.  With --storage quantized the handle is the quantized one (PATH is its file).  A/B legs are separate processes:
NMN_HNSW_NO_COALESCE=1 makes callers take turns, NEUMANN_GPU_LIB=<an older build> is the baseline (entries that build lacks are
left unbound, and its coalesce figures read null).  With --metric NAME (an ExtendedDistanceMetric) the callers call
nmn_hnsw_search_metric(nq = 1) under that metric instead, top_k taken in turn from 1, 10, 50, 100 (docs/hnsw.md §12).

  python tools/hnsw_bench.py --rows 200000 --dim 128 --sparse-queries 0.8 --index-file PATH
--sparse-queries FRACTION zeroes that share of every synthetic query's entries and times nmn_hnsw_search_sparse beside
nmn_hnsw_search of the SAME (densified) queries, the two alternating call by call, at 1 / 64 / 1024 queries per call and ef 50 /
200 (docs/hnsw.md §13): medians of --calls (a fifth of it at 1024 queries), spread over --repeats.  Both are host-buffer calls,
so both figures are wall times of the whole call, copies included (--sparse-device times the device-buffer entry).  It also
prints the stored entries per query, the evaluations per query and the queries the spill launch answered, and checks that the
sparse call's device and host-walk answers are the same bits and, under Euclidean, the bits of the dense walk.

  timeout -k 10 900 python tools/hnsw_bench.py --rows 200000 --dim 128 --sparse-device --index-file PATH   # once per repetition
--sparse-device times nmn_hnsw_search_sparse_device (docs/hnsw.md §22) on the queries of --sparse-queries' recipe (--sparse-fraction
of every entry zeroed, 0.8 by default) held as a CSR in device memory, at 1 / 64 / 1024 queries per call, k = --k, ef 50.  Three calls
alternate call by call on the same handle: search_sparse_device between two events, search_device of the densified queries
between two events — the walk without the canonicaliser and the kind-1 scoring — and the host-buffer search_sparse by wall time;
medians of --calls.  One repetition per process: run it --repeats times, each under its own time limit, and take the spread over
the lines.  It ends the run unless the device and host answers of the first 64 queries are the same bits.

  python tools/hnsw_bench.py --rows 200000 --dim 128 --sparse-callers 64,128 --index-file PATH [--storage quantized]
--sparse-callers times CONCURRENT sparse callers (docs/hnsw.md §14): for every T of the list, T threads behind a barrier, each making
--caller-calls calls of nmn_hnsw_search_sparse with ONE query (--sparse-fraction of its entries zeroed, 0.8 by default: about a fifth
of the dimension stored), k taken in turn from 1, 10, 50, 100.  The run alternates two legs, --repeats times: the build as it is, and
the same build with NMN_HNSW_NO_COALESCE=1, where sparse callers take turns on the handle — what they did before they joined the
coalescer.  Every leg is a fresh child process (this script again, with --sparse-leg) under its own time limit (--leg-timeout
seconds); with --index-file the first leg builds and saves the index and every other leg loads it.  One JSON line per leg (queries_per_s,
call_ms_median, merged batches and calls from nmn_hnsw_coalesce_stats), then one line with the medians and spreads of both legs.

  python tools/hnsw_bench.py --rows 200000 --dim 128 --cache-callers 64,128 [--cache-metric cosine] --index-file PATH
--cache-callers times CONCURRENT semantic-cache lookups (docs/hnsw.md §16): for every T of the list, T threads behind a barrier, each
making --caller-calls calls of nmn_hnsw_cache_search with ONE query, k = 1 and threshold 0.9 under --cache-metric — the call
CacheIndex::search_with_metric makes for every lookup.  The legs are --sparse-callers': this build, and this build under
NMN_HNSW_NO_COALESCE=1, alternating, each a fresh child process (this script again, with --cache-leg) under --leg-timeout.

  python tools/hnsw_bench.py --rows 200000 --dim 128 --bulk-build [--bulk-policy BATCH,MIN_NODES]
--bulk-build times the BUILD and nothing else (docs/hnsw.md §19): --repeats legs, each a fresh child process (this script again,
with --bulk-leg) under --leg-timeout that builds the same rows with nmn_hnsw_insert and with nmn_hnsw_insert_bulk on fresh
handles in 50 000-row calls — the order of the two alternating leg by leg — saves both and ends the run unless the two files are
byte-equal.  One JSON line per leg: insert_build_s and bulk_build_s, the seconds of every call of either (the graph grows from call
to call), nmn_hnsw_get_bulk_stats, the accepted share, the batch-size trace (a histogram, and its first runs run-length coded)
and the split of the bulk build into walk launches, validation plus commits, and patches; then one line with medians and spreads.

  timeout -k 10 1100 python tools/hnsw_bench.py --rows 200000 --dim 128 --tt-queries 4,4,8:8 --tt-node-fraction 0.5   # once per repetition
--tt-node-fraction F (docs/hnsw.md §24): Gaussian trains of --tt-queries' SHAPE:RANK, a share F of them inserted as TensorTrain
nodes (nmn_hnsw_insert_embedding_tt) and the others as Dense(reconstruction), beside a second handle over the same reconstructions
as Dense nodes only — the yardstick, built in the same process.  search_tt_device and search_device alternate call by call on both
handles between events at 1, 64 and 1 024 queries; the device, host-buffer and host-walk answers of the handle with TT nodes must
be the same bits.  One JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def time_rerank(g, xmetric, Q, qd, k, s, args):
    """device time of search_metric_device (top_k = k) and of search_device at k = c and the index's ef_search: the walk alone"""
    import torch
    c = min(max(2 * k, 10), max(len(g), 1))
    ef = g.config.ef_search  # what search_metric_device walks with: the two columns are the same walk under every preset
    r = {"top_k": k, "c": c, "ef": ef}
    bufs = {}
    for nq in (1, 64, 1024):
        bufs[nq] = tuple((torch.empty((nq, kk), dtype=torch.int64, device="cuda"), torch.empty((nq, kk), dtype=torch.float32, device="cuda"),
                          torch.empty((nq,), dtype=torch.int32, device="cuda")) for kk in (k, c))
        g.search_metric_device(qd[:nq], k, xmetric, out=bufs[nq][0], stream=s)  # warm every shape
        g.search_device(qd[:nq], c, ef, out=bufs[nq][1], stream=s)
    s.synchronize()
    got = g.search_metric(Q[:64], k, xmetric, with_stats=True)
    r["device_and_host_buffers_agree"] = bool(
        np.array_equal(bufs[64][0][0].cpu().numpy().view(np.uint64), got[0]) and
        np.array_equal(bufs[64][0][1].cpu().numpy().view(np.uint32), got[1].view(np.uint32)))
    r["candidates_rescored"] = int(got[3].candidates_rescored)
    reps = {}
    for _ in range(args.repeats):
        for nq, calls in ((1, args.calls), (64, args.calls), (1024, max(args.calls // 5, 5))):
            ev_m, ev_w = [], []
            for _ in range(calls):  # the two alternate call by call: both see the same machine state
                e = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
                e[0].record(s)
                g.search_metric_device(qd[:nq], k, xmetric, out=bufs[nq][0], stream=s)
                e[1].record(s)
                e[2].record(s)
                g.search_device(qd[:nq], c, ef, out=bufs[nq][1], stream=s)
                e[3].record(s)
                ev_m.append((e[0], e[1]))
                ev_w.append((e[2], e[3]))
            s.synchronize()
            reps.setdefault(f"metric_dev_ms_per_call_nq{nq}", []).append(float(np.median([a.elapsed_time(b) for a, b in ev_m])))
            reps.setdefault(f"walk_dev_ms_per_call_nq{nq}", []).append(float(np.median([a.elapsed_time(b) for a, b in ev_w])))
    for key, v in reps.items():
        r[key] = round(float(np.median(v)), 5)
        r[key + "_spread"] = round(float((max(v) - min(v)) / np.median(v)), 3)
    for nq in (1, 64, 1024):
        r[f"rerank_extra_ms_per_call_nq{nq}"] = round(r[f"metric_dev_ms_per_call_nq{nq}"] - r[f"walk_dev_ms_per_call_nq{nq}"], 5)
    return r


def time_storage(gq, gd, Q, qd, k, s, args, metric, tag="q8"):
    """the quantized (tag "q8") or binary (tag "bin") walk beside the dense walk of the same corpus, alternating call by call"""
    import torch
    out = {}
    flat = gd.vectors()
    ex_rows, _, _ = flat.search(Q, k, metric)
    for ef in (50, 200):
        r = {}
        bufs = {}
        for nq in (1, 64, 1024):
            bufs[nq] = tuple((torch.empty((nq, k), dtype=torch.int64, device="cuda"), torch.empty((nq, k), dtype=torch.float32, device="cuda"),
                              torch.empty((nq,), dtype=torch.int32, device="cuda")) for _ in range(2))
            gq.search_device(qd[:nq], k, ef, out=bufs[nq][0], stream=s)  # warm every shape
            gd.search_device(qd[:nq], k, ef, out=bufs[nq][1], stream=s)
            gq.search(Q[:nq], k, ef)
            gd.search(Q[:nq], k, ef)
        s.synchronize()
        for name, g, b in ((tag, gq, 0), ("dense", gd, 1)):
            ids, sc, cnt, st = g.search(Q, k, ef, with_stats=True)
            r[f"{name}_evals_per_query"] = round(st.rows_scanned / len(Q), 1)
            r[f"{name}_spilled_queries"] = int(st.fallback_queries)
            r[f"{name}_recall_at_{k}"] = round(float(np.mean([len(set(a.tolist()) & set(e.tolist())) / k for a, e in zip(ids, ex_rows)])), 4)
            same = np.array_equal(bufs[1024][b][0].cpu().numpy().view(np.uint64), ids) and \
                np.array_equal(bufs[1024][b][1].cpu().numpy().view(np.uint32), sc.view(np.uint32))
            if name == tag:
                os.environ["NMN_HNSW_HOST_SEARCH"] = "1"
                try:
                    hids, hsc, _ = g.search(Q[:64], k, ef)
                finally:
                    del os.environ["NMN_HNSW_HOST_SEARCH"]
                same = same and np.array_equal(hids, ids[:64]) and np.array_equal(hsc.view(np.uint32), sc[:64].view(np.uint32))
            r[f"{name}_paths_agree"] = bool(same)
        reps = {}
        for _ in range(args.repeats):
            for nq, calls in ((1, args.calls), (64, args.calls), (1024, max(args.calls // 5, 5))):
                ev = {tag: [], "dense": []}
                for _ in range(calls):
                    e = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
                    e[0].record(s)
                    gq.search_device(qd[:nq], k, ef, out=bufs[nq][0], stream=s)
                    e[1].record(s)
                    e[2].record(s)
                    gd.search_device(qd[:nq], k, ef, out=bufs[nq][1], stream=s)
                    e[3].record(s)
                    ev[tag].append((e[0], e[1]))
                    ev["dense"].append((e[2], e[3]))
                s.synchronize()
                for name in ev:
                    reps.setdefault(f"{name}_dev_ms_per_query_nq{nq}", []).append(float(np.median([a.elapsed_time(b) for a, b in ev[name]])) / nq)
            tq, td = [], []
            for _ in range(args.calls):
                t0 = time.perf_counter()
                gq.search(Q[:1], k, ef)
                t1 = time.perf_counter()
                gd.search(Q[:1], k, ef)
                t2 = time.perf_counter()
                tq.append(t1 - t0)
                td.append(t2 - t1)
            reps.setdefault(f"{tag}_gpu_ms_nq1", []).append(float(np.median(tq)) * 1e3)
            reps.setdefault("dense_gpu_ms_nq1", []).append(float(np.median(td)) * 1e3)
        for key, v in reps.items():
            r[key] = round(float(np.median(v)), 5)
            r[key + "_spread"] = round(float((max(v) - min(v)) / np.median(v)), 3)
        for nq in (1, 64, 1024):
            r[f"{tag}_over_dense_nq{nq}"] = round(r[f"{tag}_dev_ms_per_query_nq{nq}"] / r[f"dense_dev_ms_per_query_nq{nq}"], 3)
        out[f"ef{ef}"] = r
    return out


def time_callers(g, Q, counts, args, xmetric=None, sparse=None, cache=None):
    """N threads, each calling g.search(one query, its k) --caller-calls times — with `xmetric`, g.search_metric(one query, its top_k,
    xmetric); with `sparse` (one CSR per query of Q), g.search_sparse(that query, its k); with `cache` (an ExtendedDistanceMetric),
    g.cache_search(one query, 1, 0.9, cache) —: throughput, a caller's median, the coalescer's counts"""
    import threading
    ks = (1, 10, 50, 100)
    has_stats = hasattr(g._lib, "nmn_hnsw_coalesce_stats")  # (an older build has no coalescer)
    out = {}
    for N in counts:
        per = args.caller_calls
        reps = {}
        for _ in range(args.repeats + 1):  # the first pass warms every shape and is dropped
            lat = [[] for _ in range(N)]
            errs = []
            start = threading.Barrier(N + 1)

            def work(t):
                try:
                    start.wait()
                    for j in range(per):
                        q = Q[(t * per + j) % len(Q)]
                        t0 = time.perf_counter()
                        if cache is not None:
                            g.cache_search(q, 1, 0.9, cache)
                        elif sparse is not None:
                            g.search_sparse(*sparse[(t * per + j) % len(Q)], ks[(t + j) % len(ks)])
                        elif xmetric is not None:
                            g.search_metric(q, ks[(t + j) % len(ks)], xmetric)
                        else:
                            g.search(q, ks[(t + j) % len(ks)])
                        lat[t].append(time.perf_counter() - t0)
                except Exception as e:  # noqa: BLE001
                    errs.append(e)

            th = [threading.Thread(target=work, args=(t,)) for t in range(N)]
            for x in th:
                x.start()
            b0 = g.coalesce_stats() if has_stats else None
            start.wait()
            t0 = time.perf_counter()
            for x in th:
                x.join()
            wall = time.perf_counter() - t0
            if errs:
                raise errs[0]
            m = {"queries_per_s": N * per / wall, "call_ms_median": float(np.median(np.concatenate(lat))) * 1e3}
            if has_stats:
                b1 = g.coalesce_stats()
                m["merged_batches"], m["merged_calls"] = b1[0] - b0[0], b1[1] - b0[1]
                m["calls_per_merged_batch"] = (b1[1] - b0[1]) / max(b1[0] - b0[0], 1)
            for key, v in m.items():
                reps.setdefault(key, []).append(v)
        r = {}
        for key, v in reps.items():
            v = v[1:]
            r[key] = round(float(np.median(v)), 4)
            r[key + "_spread"] = round(float((max(v) - min(v)) / max(np.median(v), 1e-12)), 3)
        if not has_stats:
            r["merged_batches"] = r["merged_calls"] = None
        out[f"callers{N}"] = r
    return out


def sparse_caller_legs(args, flag="--sparse-leg"):
    """--sparse-callers / --cache-callers: the two legs alternating, each a fresh child process with its own time limit; this process
    opens no GPU"""
    import subprocess
    argv = [sys.executable, os.path.abspath(__file__), flag] + [a for a in sys.argv[1:] if a != flag]
    legs = {"coalesce": [], "no_coalesce": []}
    for _ in range(args.repeats):
        for leg in legs:
            env = dict(os.environ)
            env.pop("NMN_HNSW_NO_COALESCE", None)
            if leg == "no_coalesce":
                env["NMN_HNSW_NO_COALESCE"] = "1"
            try:
                r = subprocess.run(argv, env=env, capture_output=True, text=True, timeout=args.leg_timeout)
            except subprocess.TimeoutExpired:
                raise SystemExit(f"leg {leg} did not end within {args.leg_timeout} s")
            if r.returncode != 0:
                raise SystemExit(f"leg {leg} ended with {r.returncode}: {r.stderr[-2000:]}")
            line = json.loads(r.stdout.strip().splitlines()[-1])
            line["leg"] = leg
            print(json.dumps(line), flush=True)
            legs[leg].append(line)
    out = {"summary": True, "rows": args.rows, "dim": args.dim, "storage": args.storage, "repeats": args.repeats}
    for leg, lines in legs.items():
        for key in [k for k in lines[0] if k.startswith("callers")]:
            r = {}
            for f in ("queries_per_s", "call_ms_median", "merged_batches", "merged_calls", "calls_per_merged_batch"):
                v = [x[key][f] for x in lines]
                r[f] = round(float(np.median(v)), 4)
                r[f + "_spread"] = round(float((max(v) - min(v)) / max(np.median(v), 1e-12)), 3)
            out[f"{leg}_{key}"] = r
    print(json.dumps(out), flush=True)


def bulk_build_legs(args):
    """--bulk-build: `repeats` legs, each a fresh child process with its own time limit that builds the same rows with
    nmn_hnsw_insert and with nmn_hnsw_insert_bulk (the order alternating leg by leg); this process opens no GPU"""
    import subprocess
    argv = [sys.executable, os.path.abspath(__file__), "--bulk-leg"] + [a for a in sys.argv[1:] if a != "--bulk-leg"]
    lines = []
    for i in range(args.repeats):
        try:
            r = subprocess.run(argv + (["--bulk-first"] if i % 2 else []), stdout=subprocess.PIPE, text=True, timeout=args.leg_timeout)
        except subprocess.TimeoutExpired:
            raise SystemExit(f"leg {i} did not end within {args.leg_timeout} s")
        if r.returncode != 0:
            raise SystemExit(f"leg {i} ended with {r.returncode}")
        line = json.loads(r.stdout.strip().splitlines()[-1])
        print(json.dumps(line), flush=True)
        lines.append(line)
    out = {"summary": True, "rows": args.rows, "dim": args.dim, "preset": args.preset, "metric": args.metric, "repeats": args.repeats,
           "bulk_policy": args.bulk_policy, "files_byte_equal": all(x["files_byte_equal"] for x in lines)}
    for f in ("insert_build_s", "bulk_build_s", "walk_s", "commit_s", "patch_s", "accepted_share"):
        v = [x[f] for x in lines]
        out[f] = round(float(np.median(v)), 3)
        out[f + "_spread"] = round(float((max(v) - min(v)) / max(np.median(v), 1e-12)), 3)
    out["speedup_of_medians"] = round(out["insert_build_s"] / max(out["bulk_build_s"], 1e-9), 3)
    print(json.dumps(out), flush=True)


def bulk_build_leg(n, d, cfg, args, out):
    """one leg of --bulk-build: both builds on fresh handles in 50 000-row calls, the two saved files compared byte for byte"""
    import filecmp
    import tempfile
    from neumann_amd import GpuHnsw, synth_rows
    step = 50_000
    tmp = tempfile.mkdtemp(prefix="hnsw_bulk_")
    paths = {}
    try:
        for which in (("bulk", "insert") if args.bulk_first else ("insert", "bulk")):
            trace, call_s = [], []
            with GpuHnsw(d, cfg, capacity_hint=n) as g:
                t0 = time.perf_counter()
                for r0 in range(0, n, step):
                    rows = synth_rows(0x2F6, r0, min(step, n - r0), d)
                    t1 = time.perf_counter()
                    if which == "bulk":
                        g.set_bulk_policy(*[int(x) for x in args.bulk_policy.split(",")])
                        g.insert_bulk(rows)
                        trace.append(g.bulk_trace())
                    else:
                        g.insert(rows)
                    call_s.append(round(time.perf_counter() - t1, 2))
                    print(f"{which}: built {min(r0 + step, n)} nodes in {time.perf_counter() - t0:.1f} s", file=sys.stderr, flush=True)
                out[which + "_build_s"] = round(time.perf_counter() - t0, 2)
                out[which + "_call_s"] = call_s  # seconds of every 50 000-row call: the graph grows from call to call
                if which == "bulk":
                    out["bulk_call_accepted_share"] = [round(float((t[:, 0] - t[:, 1]).sum() / max(t[:, 0].sum(), 1)), 3) for t in trace]
                    out["bulk_call_mean_batch"] = [round(float(t[:, 0].mean()), 1) if len(t) else 0.0 for t in trace]
                    out["bulk_call_walk_s"] = [round(float(t[:, 2].sum()) / 1e3, 2) for t in trace]
                    st = g.bulk_stats()
                    tr = np.concatenate(trace) if trace else np.zeros((0, 5), np.float32)
                    out["bulk_stats"] = st
                    out["accepted_share"] = round(st["accepted"] / max(st["walks"], 1), 4)
                    out["walk_s"], out["commit_s"], out["patch_s"] = (round(float(tr[:, c].sum()) / 1e3, 3) for c in (2, 3, 4))
                    sizes = tr[:, 0].astype(int)
                    out["batch_size_histogram"] = {str(int(b)): int((sizes == b).sum()) for b in np.unique(sizes)}
                    runs = []  # the trace run-length coded: [size, batches in a row]
                    for b in sizes.tolist():
                        if runs and runs[-1][0] == b:
                            runs[-1][1] += 1
                        else:
                            runs.append([b, 1])
                    out["batch_size_runs"] = runs[:48]
                    out["batch_size_runs_total"] = len(runs)
                paths[which] = os.path.join(tmp, which + ".idx")
                g.save(paths[which])
        out["files_byte_equal"] = filecmp.cmp(paths["insert"], paths["bulk"], shallow=False)
        out["index_file_bytes"] = os.path.getsize(paths["bulk"])
    finally:
        for pth in paths.values():
            if os.path.exists(pth):
                os.remove(pth)
        os.rmdir(tmp)
    if not out["files_byte_equal"]:
        print(json.dumps(out), flush=True)
        raise SystemExit("--bulk-build: the two saved indexes differ")
    return out


def time_sparse(g, Q, k, args):
    """nmn_hnsw_search_sparse beside nmn_hnsw_search of the densified queries, host buffers, alternating call by call"""
    rng = np.random.default_rng(0x5BA)
    Q = Q.copy()
    Q[rng.random(Q.shape) < args.sparse_queries] = 0.0
    csr = g.sparse_from_dense(Q)
    out = {"sparse_fraction": args.sparse_queries, "entries_per_query": round(float(csr[1].size) / Q.shape[0], 1)}

    def part(nq):
        e = int(csr[0][nq])
        return csr[0][:nq + 1], csr[1][:e], csr[2][:e]

    for ef in (50, 200):
        r = {}
        for nq in (1, 64, 1024):  # warm every shape
            g.search_sparse(*part(nq), k, ef)
            g.search(Q[:nq], k, ef)
        ids, sc, cnt, st = g.search_sparse(*csr, k, ef, with_stats=True)
        r["evals_per_query"] = round(st.rows_scanned / Q.shape[0], 1)
        r["spilled_queries"] = int(st.fallback_queries)
        dids, dsc, _ = g.search(Q, k, ef)
        r["queries_whose_score_bits_differ_from_the_dense_walk"] = int((sc.view(np.uint32) != dsc.view(np.uint32)).any(axis=1).sum())
        os.environ["NMN_HNSW_HOST_SEARCH"] = "1"
        try:
            hids, hsc, _ = g.search_sparse(*part(64), k, ef)
        finally:
            del os.environ["NMN_HNSW_HOST_SEARCH"]
        r["device_and_host_walk_agree"] = bool(np.array_equal(hids, ids[:64]) and np.array_equal(hsc.view(np.uint32), sc[:64].view(np.uint32)))
        if int(g.config.distance_metric) == 1:
            r["equals_the_dense_walk"] = bool(np.array_equal(dids, ids) and np.array_equal(dsc.view(np.uint32), sc.view(np.uint32)))
        reps = {}
        for _ in range(args.repeats):
            for nq, calls in ((1, args.calls), (64, args.calls), (1024, max(args.calls // 5, 5))):
                p, qs = part(nq), Q[:nq]
                ts, td = [], []
                for _ in range(calls):
                    t0 = time.perf_counter()
                    g.search_sparse(*p, k, ef)
                    t1 = time.perf_counter()
                    g.search(qs, k, ef)
                    t2 = time.perf_counter()
                    ts.append(t1 - t0)
                    td.append(t2 - t1)
                reps.setdefault(f"sparse_ms_per_call_nq{nq}", []).append(float(np.median(ts)) * 1e3)
                reps.setdefault(f"dense_ms_per_call_nq{nq}", []).append(float(np.median(td)) * 1e3)
        for key, v in reps.items():
            r[key] = round(float(np.median(v)), 5)
            r[key + "_spread"] = round(float((max(v) - min(v)) / np.median(v)), 3)
        out[f"ef{ef}"] = r
    return out


def time_mixed(n, d, cfg, Q, k, args, out):
    """--sparse-node-fraction F (docs/hnsw.md §15): a handle where a share F of the rows is inserted Sparse (70 % of the elements of
    such a row zeroed, the others doubled) beside an all-dense handle over the to_dense() rows, both built here; search_device and
    search_sparse of either, alternating call by call; the mixed handle's device, host-buffer and host-walk answers compared bit
    for bit."""
    import torch
    from neumann_amd import GpuHnsw, synth_rows
    rng = np.random.default_rng(0x15A)
    F = args.sparse_node_fraction
    with GpuHnsw(d, cfg, capacity_hint=n) as gm, GpuHnsw(d, cfg, capacity_hint=n) as gd:
        t0 = time.perf_counter()
        step = 10_000
        for r0 in range(0, n, step):
            rows = synth_rows(0x2F6, r0, min(step, n - r0), d).copy()
            sparse = rng.random(len(rows)) < F
            rows[sparse] = np.where(rng.random((int(sparse.sum()), d)) < 0.7, np.float32(0), rows[sparse] * np.float32(2))
            i = 0
            while i < len(rows):  # runs of one kind, in row order
                j = i
                while j < len(rows) and sparse[j] == sparse[i]:
                    j += 1
                if sparse[i]:
                    gm.insert_sparse(*gm.sparse_from_dense(rows[i:j]))
                else:
                    gm.insert(rows[i:j])
                i = j
            gd.insert(rows)  # (to_dense(from_dense(row)) is the row: synth rows hold no -0.0)
            print(f"built {min(r0 + step, n)} nodes of both handles in {time.perf_counter() - t0:.1f} s", file=sys.stderr, flush=True)
        out["build_s_both"] = round(time.perf_counter() - t0, 1)
        ms = gm.memory_stats()
        out.update({"sparse_node_fraction": F, "sparse_nodes": ms["sparse_count"], "dense_nodes": ms["dense_count"],
                    "hbm_bytes_mixed": gm.hbm_bytes, "hbm_bytes_dense": gd.hbm_bytes})
        Qs = Q.copy()
        Qs[rng.random(Qs.shape) < 0.8] = 0.0
        csr = gm.sparse_from_dense(Qs)
        qd = torch.from_numpy(Q).cuda()

        def part(nq):
            e = int(csr[0][nq])
            return csr[0][:nq + 1], csr[1][:e], csr[2][:e]

        def host(res):
            torch.cuda.synchronize()
            return res[0].cpu().numpy().view(np.uint64), res[1].cpu().numpy(), res[2].cpu().numpy().astype(np.uint32)

        def same(a, b):
            return bool(np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32)) and np.array_equal(a[2], b[2]))

        ef = 50
        dev_ans = host(gm.search_device(qd[:64], k, ef))
        buf_ans = gm.search(Q[:64], k, ef)
        sp_ans = gm.search_sparse(*part(64), k, ef)
        os.environ["NMN_HNSW_HOST_SEARCH"] = "1"
        try:
            walk_ans = gm.search(Q[:64], k, ef)
            walk_sp = gm.search_sparse(*part(64), k, ef)
        finally:
            del os.environ["NMN_HNSW_HOST_SEARCH"]
        out["device_and_host_buffer_agree"] = same(dev_ans, buf_ans)
        out["device_and_host_walk_agree"] = same(buf_ans, walk_ans)
        out["sparse_device_and_host_walk_agree"] = same(sp_ans, walk_sp)
        dd = gd.search(Q[:64], k, ef)
        out["answers_that_differ_from_the_all_dense_handle"] = int(((buf_ans[0] != dd[0]) | (buf_ans[1].view(np.uint32) != dd[1].view(np.uint32))).any(axis=1).sum())
        reps = {}
        for nq in (1, 64, 1024):  # warm every shape
            for g in (gm, gd):
                g.search_device(qd[:nq], k, ef)
                g.search_sparse(*part(nq), k, ef)
        torch.cuda.synchronize()
        for _ in range(args.repeats):
            for nq, calls in ((1, args.calls), (64, args.calls), (1024, max(args.calls // 5, 5))):
                p, q = part(nq), qd[:nq]
                t = {"mixed_device": [], "dense_device": [], "mixed_sparse": [], "dense_sparse": []}
                for _ in range(calls):
                    for name, g in (("mixed", gm), ("dense", gd)):
                        t0 = time.perf_counter()
                        g.search_device(q, k, ef)
                        torch.cuda.synchronize()
                        t1 = time.perf_counter()
                        g.search_sparse(*p, k, ef)
                        t2 = time.perf_counter()
                        t[name + "_device"].append(t1 - t0)
                        t[name + "_sparse"].append(t2 - t1)
                for name, v in t.items():
                    reps.setdefault(f"{name}_ms_per_call_nq{nq}", []).append(float(np.median(v)) * 1e3)
        for key, v in reps.items():
            out[key] = round(float(np.median(v)), 5)
            out[key + "_spread"] = round(float((max(v) - min(v)) / np.median(v)), 3)
    return out


def build_or_load(path, n, d, cfg, storage, out, label="", binary_threshold=None):
    """the handle of the run: GpuHnsw.load(path) when the file exists; otherwise built by nmn_hnsw_insert and, with a path, saved
    and loaded back once.  Seconds and file bytes go to `out`.  (A binary handle is always built: it has no file form, path None.)"""
    from neumann_amd import GpuHnsw, synth_rows
    pre = f"{label}_" if label else ""
    if path and os.path.exists(path):
        t0 = time.perf_counter()
        g = GpuHnsw.load(path, capacity_hint=n)
        out[pre + "load_s"] = round(time.perf_counter() - t0, 3)
        out[pre + "index_file_bytes"] = os.path.getsize(path)
        have = (len(g), g.dim, g.storage, g.config.m, g.config.m0, g.config.ef_construction, g.config.ef_search, int(g.config.distance_metric))
        want = (n, d, storage, cfg.m, cfg.m0, cfg.ef_construction, cfg.ef_search, int(cfg.distance_metric))
        if have != want:
            g.close()
            raise SystemExit(f"{path} holds another index: (rows, dim, storage, m, m0, ef_construction, ef_search, metric) = {have}, asked for {want}")
        print(f"{pre}loaded {n} nodes from {path} in {out[pre + 'load_s']} s", file=sys.stderr, flush=True)
        return g
    g = GpuHnsw(d, cfg, capacity_hint=n, storage=storage, binary_threshold=binary_threshold)
    t0 = time.perf_counter()
    step = 50_000
    for r0 in range(0, n, step):
        g.insert(synth_rows(0x2F6, r0, min(step, n - r0), d))
        print(f"{pre}built {min(r0 + step, n)} nodes in {time.perf_counter() - t0:.1f} s", file=sys.stderr, flush=True)
    out[pre + "build_s"] = round(time.perf_counter() - t0, 1)
    if path:
        t0 = time.perf_counter()
        g.save(path)
        out[pre + "save_s"] = round(time.perf_counter() - t0, 3)
        out[pre + "index_file_bytes"] = os.path.getsize(path)
        t0 = time.perf_counter()
        with GpuHnsw.load(path) as g2:
            out[pre + "load_s"] = round(time.perf_counter() - t0, 3)
            if (len(g2), g2.entry_point, g2.max_layer) != (len(g), g.entry_point, g.max_layer):
                raise SystemExit(f"{path} did not load as it was saved")
    return g


def time_tt(g, k, args):
    """--tt-queries SHAPE:RANK (docs/hnsw.md §17): 1024 Gaussian trains of that shape with every inner rank RANK.  search_tt_device
    (preparation + walk) against search_device of the same number of dense queries — the trains' reconstructions — on the same
    handle and stream, alternating call by call, each call between two events; the difference is the preparation's cost.  Device,
    host-buffer and host-walk answers of the first 64 trains must be the same bits."""
    import torch
    from neumann_amd import TTVector, tt_reconstruct
    shape_s, rank_s = args.tt_queries.split(":")
    shape = [int(x) for x in shape_s.split(",")]
    ranks = [1] + [int(rank_s)] * (len(shape) - 1) + [1]
    sizes = [ranks[i] * shape[i] * ranks[i + 1] for i in range(len(shape))]
    rng = np.random.default_rng(0x77B)
    cores = rng.standard_normal((1024, sum(sizes))).astype(np.float32)
    cuts = np.cumsum([0] + sizes)
    tts = [TTVector(shape, ranks, [row[cuts[i]:cuts[i + 1]] for i in range(len(shape))]) for row in cores]
    Q = tt_reconstruct(tts)
    s = torch.cuda.Stream()
    cd, qd = torch.from_numpy(cores).cuda(), torch.from_numpy(Q).cuda()
    r = {"tt_shape": shape, "tt_ranks": ranks, "core_floats": int(sum(sizes))}
    dev = {}
    for nq in (1, 64, 1024):
        dev[nq] = tuple((torch.empty((nq, k), dtype=torch.int64, device="cuda"), torch.empty((nq, k), dtype=torch.float32, device="cuda"),
                         torch.empty((nq,), dtype=torch.int32, device="cuda")) for _ in range(2))
        g.search_tt_device(shape, ranks, cd[:nq], k, 50, out=dev[nq][0], stream=s)
        g.search_device(qd[:nq], k, 50, out=dev[nq][1], stream=s)
    s.synchronize()
    ids, sc, _ = g.search_tt(tts[:64], k, 50)
    same = np.array_equal(dev[64][0][0].cpu().numpy().view(np.uint64), ids) and \
        np.array_equal(dev[64][0][1].cpu().numpy().view(np.uint32), sc.view(np.uint32))
    os.environ["NMN_HNSW_HOST_SEARCH"] = "1"
    try:
        hids, hsc, _ = g.search_tt(tts[:64], k, 50)
    finally:
        del os.environ["NMN_HNSW_HOST_SEARCH"]
    same = same and np.array_equal(hids, ids) and np.array_equal(hsc.view(np.uint32), sc.view(np.uint32))
    r["device_host_buffer_and_host_walk_agree"] = bool(same)
    if not same:
        raise SystemExit("search_tt_device, search_tt and the host walk disagree")
    for nq, calls in ((1, args.calls), (64, args.calls), (1024, max(args.calls // 5, 5))):
        tt_ev, de_ev = [], []
        for _ in range(calls):
            e0, e1, e2 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
            e0.record(s)
            g.search_tt_device(shape, ranks, cd[:nq], k, 50, out=dev[nq][0], stream=s)
            e1.record(s)
            g.search_device(qd[:nq], k, 50, out=dev[nq][1], stream=s)
            e2.record(s)
            tt_ev.append((e0, e1))
            de_ev.append((e1, e2))
        s.synchronize()
        t_tt = np.array([a.elapsed_time(b) for a, b in tt_ev])
        t_de = np.array([a.elapsed_time(b) for a, b in de_ev])
        r[f"nq{nq}"] = {"calls": calls, "tt_call_ms": round(float(np.median(t_tt)), 5), "dense_call_ms": round(float(np.median(t_de)), 5),
                        "preparation_call_ms": round(float(np.median(t_tt - t_de)), 5),
                        "preparation_call_ms_p10_p90": [round(float(x), 5) for x in np.percentile(t_tt - t_de, [10, 90])]}
    return r


def time_tt_nodes(n, d, cfg, k, args, out):
    """--tt-node-fraction F (docs/hnsw.md §24): n Gaussian trains of --tt-queries' SHAPE:RANK (its product must be --dim).  ONE
    process builds a handle where a share F of them — drawn per run of 500 trains, each run one insert call — is inserted as
    TensorTrain nodes (insert_embedding_tt) and the others as Dense(reconstruction), and a handle over the same reconstructions as Dense nodes only — the yardstick.  search_tt_device and
    search_device then alternate call by call on both handles, each call between two events, at 1, 64 and 1 024 queries, ef 50.
    The device, host-buffer and host-walk answers of the TT-node handle to the first 64 trains must be the same bits."""
    import torch
    from neumann_amd import GpuHnsw, TTVector, tt_reconstruct
    shape_s, rank_s = (args.tt_queries or "4,4,8:8").split(":")
    shape = [int(x) for x in shape_s.split(",")]
    if int(np.prod(shape)) != d:
        raise SystemExit(f"--tt-queries {shape_s}: the product of the shape must be --dim {d}")
    ranks = [1] + [int(rank_s)] * (len(shape) - 1) + [1]
    sizes = [ranks[i] * shape[i] * ranks[i + 1] for i in range(len(shape))]
    cuts = np.cumsum([0] + sizes)
    rng = np.random.default_rng(0x77C)

    def trains(cores):
        return [TTVector(shape, ranks, [row[cuts[i]:cuts[i + 1]] for i in range(len(shape))]) for row in cores]

    F = args.tt_node_fraction
    r = dict(out, tt_shape=shape, tt_ranks=ranks, core_floats=int(sum(sizes)), tt_node_fraction=F)
    with GpuHnsw(d, cfg, capacity_hint=n) as gt, GpuHnsw(d, cfg, capacity_hint=n) as gd:
        t0 = time.perf_counter()
        step, n_tt = 2_000, 0
        for r0 in range(0, n, step):
            cores = rng.standard_normal((min(step, n - r0), sum(sizes))).astype(np.float32)
            ts = trains(cores)
            rows = tt_reconstruct(ts)
            as_tt = np.repeat(rng.random(-(-len(ts) // 500)) < F, 500)[:len(ts)]   # the kind is drawn per run of 500 trains
            i = 0
            while i < len(ts):          # runs of one kind, each one call, in row order
                j = i
                while j < len(ts) and as_tt[j] == as_tt[i]:
                    j += 1
                gt.insert_embedding_tt(ts[i:j]) if as_tt[i] else gt.insert(rows[i:j])
                i = j
            gd.insert(rows)
            n_tt += int(as_tt.sum())
            print(f"built {min(r0 + step, n)} nodes of both handles in {time.perf_counter() - t0:.1f} s", file=sys.stderr, flush=True)
        r["build_both_s"] = round(time.perf_counter() - t0, 3)
        r["tt_nodes"], r["walk_limits"] = n_tt, list(gt.tt_walk_limits(50))
        r["hbm_bytes_tt_handle"], r["hbm_bytes_dense_handle"] = gt.hbm_bytes, gd.hbm_bytes
        qcores = rng.standard_normal((1024, sum(sizes))).astype(np.float32)
        tq = trains(qcores)
        Q = tt_reconstruct(tq)
        s = torch.cuda.Stream()
        cd, qd = torch.from_numpy(qcores).cuda(), torch.from_numpy(Q).cuda()
        bufs = {nq: tuple((torch.empty((nq, k), dtype=torch.int64, device="cuda"), torch.empty((nq, k), dtype=torch.float32, device="cuda"),
                           torch.empty((nq,), dtype=torch.int32, device="cuda")) for _ in range(4)) for nq in (1, 64, 1024)}
        legs = (("tt_nodes_tt", gt, True), ("tt_nodes_dense", gt, False), ("dense_nodes_tt", gd, True), ("dense_nodes_dense", gd, False))

        def call(g, tt_query, nq, buf):
            if tt_query:
                g.search_tt_device(shape, ranks, cd[:nq], k, 50, out=buf, stream=s)
            else:
                g.search_device(qd[:nq], k, 50, out=buf, stream=s)
        for nq in bufs:
            for (_, g, tt_query), buf in zip(legs, bufs[nq]):
                call(g, tt_query, nq, buf)
        s.synchronize()
        ids, sc, _ = gt.search_tt(tq[:64], k, 50)
        same = np.array_equal(bufs[64][0][0].cpu().numpy().view(np.uint64), ids) and \
            np.array_equal(bufs[64][0][1].cpu().numpy().view(np.uint32), sc.view(np.uint32))
        os.environ["NMN_HNSW_HOST_SEARCH"] = "1"
        try:
            hids, hsc, _ = gt.search_tt(tq[:64], k, 50)
        finally:
            del os.environ["NMN_HNSW_HOST_SEARCH"]
        same = same and np.array_equal(hids, ids) and np.array_equal(hsc.view(np.uint32), sc.view(np.uint32))
        r["device_host_buffer_and_host_walk_agree"] = bool(same)
        if not same:
            raise SystemExit("search_tt_device, search_tt and the host walk disagree on the handle with TT nodes")
        for nq, calls in ((1, args.calls), (64, args.calls), (1024, max(args.calls // 5, 5))):
            ev = {name: [] for name, _, _ in legs}
            for _ in range(calls):
                for (name, g, tt_query), buf in zip(legs, bufs[nq]):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(s)
                    call(g, tt_query, nq, buf)
                    e1.record(s)
                    ev[name].append((e0, e1))
            s.synchronize()
            r[f"nq{nq}"] = {"calls": calls}
            for name in ev:
                t = np.array([a.elapsed_time(b) for a, b in ev[name]])
                r[f"nq{nq}"][name + "_call_ms"] = round(float(np.median(t)), 5)
                r[f"nq{nq}"][name + "_call_ms_p10_p90"] = [round(float(x), 5) for x in np.percentile(t, [10, 90])]
    return r


def time_sparse_device(g, Q, k, args):
    """--sparse-device (docs/hnsw.md §22): the queries of --sparse-queries' recipe (--sparse-fraction of every entry zeroed) as a CSR
    in device memory.  Three calls alternate call by call on the same handle: search_sparse_device between two events, search_device
    of the densified queries between two events — the walk without the new stage — and the host-buffer search_sparse by wall time.
    ef 50.  The device and host answers of the first 64 queries must be the same bits."""
    import torch
    rng = np.random.default_rng(0x5BA)
    Q = Q.copy()
    Q[rng.random(Q.shape) < args.sparse_fraction] = 0.0
    csr = g.sparse_from_dense(Q)
    ef = 50
    r = {"sparse_fraction": args.sparse_fraction, "entries_per_query": round(float(csr[1].size) / Q.shape[0], 1), "ef": ef}

    def part(nq):
        e = int(csr[0][nq])
        return csr[0][:nq + 1], csr[1][:e], csr[2][:e]

    s = torch.cuda.Stream()
    qd = torch.from_numpy(Q).cuda()
    dev, dcsr = {}, {}
    for nq in (1, 64, 1024):  # warm every shape
        ip, pos, val = part(nq)
        dcsr[nq] = (torch.from_numpy(ip.astype(np.int64)).cuda(), torch.from_numpy(pos.view(np.int32)).cuda(), torch.from_numpy(val).cuda())
        dev[nq] = tuple((torch.empty((nq, k), dtype=torch.int64, device="cuda"), torch.empty((nq, k), dtype=torch.float32, device="cuda"),
                         torch.empty((nq,), dtype=torch.int32, device="cuda")) for _ in range(2))
        dev[nq] += (torch.empty((nq,), dtype=torch.int32, device="cuda"),)
        g.search_sparse_device(*dcsr[nq], k, ef, out=dev[nq][0], status=dev[nq][2], stream=s)
        g.search_device(qd[:nq], k, ef, out=dev[nq][1], stream=s)
        g.search_sparse(*part(nq), k, ef)
    s.synchronize()
    ids, sc, cnt = g.search_sparse(*part(64), k, ef)
    same = np.array_equal(dev[64][0][0].cpu().numpy().view(np.uint64), ids) and \
        np.array_equal(dev[64][0][1].cpu().numpy().view(np.uint32), sc.view(np.uint32)) and \
        np.array_equal(dev[64][0][2].cpu().numpy().view(np.uint32), cnt) and not bool(dev[64][2].any())
    r["device_and_host_entries_agree"] = bool(same)
    if not same:
        raise SystemExit("search_sparse_device and search_sparse disagree")
    for nq, calls in ((1, args.calls), (64, args.calls), (1024, args.calls)):
        p = part(nq)
        sp_ev, de_ev, host = [], [], []
        for _ in range(calls):
            e0, e1, e2 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
            e0.record(s)
            g.search_sparse_device(*dcsr[nq], k, ef, out=dev[nq][0], status=dev[nq][2], stream=s)
            e1.record(s)
            g.search_device(qd[:nq], k, ef, out=dev[nq][1], stream=s)
            e2.record(s)
            s.synchronize()
            t0 = time.perf_counter()
            g.search_sparse(*p, k, ef)
            host.append((time.perf_counter() - t0) * 1e3)
            sp_ev.append((e0, e1))
            de_ev.append((e1, e2))
        t_sp = np.array([a.elapsed_time(b) for a, b in sp_ev])
        t_de = np.array([a.elapsed_time(b) for a, b in de_ev])
        r[f"nq{nq}"] = {"calls": calls, "sparse_device_call_ms": round(float(np.median(t_sp)), 5),
                        "dense_device_call_ms": round(float(np.median(t_de)), 5),
                        "sparse_minus_dense_call_ms": round(float(np.median(t_sp - t_de)), 5),
                        "sparse_minus_dense_call_ms_p10_p90": [round(float(x), 5) for x in np.percentile(t_sp - t_de, [10, 90])],
                        "host_entry_call_ms": round(float(np.median(host)), 5),
                        "host_entry_over_sparse_device": round(float(np.median(host) / np.median(t_sp)), 3)}
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--preset", default="default", choices=["default", "high_recall", "high_speed"])
    ap.add_argument("--metric", default="0", help="a number: the index's HNSWDistanceMetric; a name: time the re-rank under that ExtendedDistanceMetric")
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--b2b", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--launch-calls", type=int, default=None)
    ap.add_argument("--storage", default="dense", choices=["dense", "quantized", "binary"],
                    help="quantized / binary: time that walk beside the dense walk of the same corpus (docs/hnsw.md §9, §18)")
    ap.add_argument("--binary-threshold", default="sign", choices=["sign", "mean", "median"], help="--storage binary: the BinaryThreshold")
    ap.add_argument("--callers", default=None, help="e.g. 1,16,64,128: time that many concurrent host callers (nq = 1, mixed k) and nothing else")
    ap.add_argument("--caller-calls", type=int, default=200, help="calls every caller thread makes per repetition")
    ap.add_argument("--sparse-queries", type=float, default=None,
                    help="zero this share of every query's entries and time nmn_hnsw_search_sparse beside nmn_hnsw_search (docs/hnsw.md §13)")
    ap.add_argument("--sparse-callers", default=None,
                    help="e.g. 64,128: that many concurrent nmn_hnsw_search_sparse callers (one query each), with and without "
                         "NMN_HNSW_NO_COALESCE=1, each leg a fresh child process (docs/hnsw.md §14)")
    ap.add_argument("--sparse-fraction", type=float, default=0.8, help="--sparse-callers: the share of every query's entries that is zeroed")
    ap.add_argument("--leg-timeout", type=float, default=900.0, help="--sparse-callers: seconds a leg's child process may take")
    ap.add_argument("--sparse-leg", action="store_true", help="(one leg of --sparse-callers, in this process)")
    ap.add_argument("--cache-callers", default=None,
                    help="e.g. 64,128: that many concurrent nmn_hnsw_cache_search callers (one query, k = 1, threshold 0.9), with and "
                         "without NMN_HNSW_NO_COALESCE=1, each leg a fresh child process (docs/hnsw.md §16)")
    ap.add_argument("--cache-metric", default="cosine", help="--cache-callers: the ExtendedDistanceMetric of the re-rank, by name")
    ap.add_argument("--cache-leg", action="store_true", help="(one leg of --cache-callers, in this process)")
    ap.add_argument("--sparse-node-fraction", type=float, default=None,
                    help="insert this share of the rows Sparse (nmn_hnsw_insert_sparse) and time search_device / search_sparse of the "
                         "mixed handle beside an all-dense handle over the to_dense() rows (docs/hnsw.md §15)")
    ap.add_argument("--sparse-device", action="store_true",
                    help="time search_sparse_device against search_device of the densified queries and the host-buffer search_sparse, "
                         "alternating call by call (docs/hnsw.md §22); --sparse-fraction of every entry zeroed; one repetition per process")
    ap.add_argument("--tt-queries", default=None,
                    help="SHAPE:RANK, e.g. 4,4,8:8 — time search_tt_device against search_device with as many dense queries on the "
                         "same handle, alternating call by call (docs/hnsw.md §17); one repetition per process")
    ap.add_argument("--index-file", default=None,
                    help="load the index from this file when it exists; otherwise build, save it there and report build / save / load seconds")
    ap.add_argument("--bulk-build", action="store_true",
                    help="build the same rows with nmn_hnsw_insert and with nmn_hnsw_insert_bulk on fresh handles, check the saved files "
                         "byte-equal, and report both build_s, the bulk counters and the batch-size trace (docs/hnsw.md §19); "
                         "--repeats legs, each a fresh child process under --leg-timeout")
    ap.add_argument("--tt-node-fraction", type=float, default=None,
                    help="build a handle with that share of --tt-queries' trains (default 4,4,8:8) inserted as TensorTrain nodes beside a "
                         "handle of their reconstructions as Dense nodes, and time search_tt_device / search_device on both, alternating "
                         "(docs/hnsw.md §24); one repetition per process")
    ap.add_argument("--bulk-leg", action="store_true", help="(one leg of --bulk-build, in this process)")
    ap.add_argument("--bulk-first", action="store_true", help="(--bulk-leg: the bulk build before the sequential one)")
    ap.add_argument("--bulk-policy", default="0,0", help="--bulk-build: batch,min_nodes of nmn_hnsw_set_bulk_policy (0 = default)")
    args = ap.parse_args()
    if args.bulk_build and not args.bulk_leg:
        bulk_build_legs(args)
        return
    if args.sparse_callers and not args.sparse_leg:
        sparse_caller_legs(args)
        return
    if args.cache_callers and not args.cache_leg:
        sparse_caller_legs(args, "--cache-leg")
        return
    if args.callers:  # an older build through NEUMANN_GPU_LIB: entries it lacks stay unbound instead of failing the load
        import ctypes
        from neumann_amd import _capi
        probe = ctypes.CDLL(_capi.LIB_PATH)
        for name in [x for x in _capi.SIGNATURES if not hasattr(probe, x)]:
            del _capi.SIGNATURES[name]
    import torch
    from neumann_amd import DistanceMetric, ExtendedDistanceMetric, HNSWConfig, synth_rows

    n, d, k = args.rows, args.dim, args.k
    xmetric = None
    if args.metric.lstrip("-").isdigit():
        args.metric = int(args.metric)
    else:
        xmetric = ExtendedDistanceMetric.from_name(args.metric)
        args.metric = 0
    cfg = getattr(HNSWConfig, args.preset)().with_distance_metric(args.metric)
    metric = DistanceMetric(args.metric)
    Q = synth_rows(0x2F8, 0, 1024, d)
    out = {"rows": n, "dim": d, "preset": args.preset, "metric": args.metric, "k": k}
    if args.bulk_build:
        del out["k"]
        print(json.dumps(bulk_build_leg(n, d, cfg, args, out)), flush=True)
        return
    if args.callers:
        out.update({"storage": args.storage, "lib": os.environ.get("NEUMANN_GPU_LIB", "default"),
                    "no_coalesce": bool(os.environ.get("NMN_HNSW_NO_COALESCE")), "caller_calls": args.caller_calls})
        del out["k"]
        with build_or_load(args.index_file, n, d, cfg, args.storage, out) as g:
            if xmetric is not None:
                out["xmetric"] = xmetric.name
            out.update(time_callers(g, Q, [int(x) for x in args.callers.split(",")], args, xmetric))
        print(json.dumps(out), flush=True)
        return
    if args.cache_callers:  # one leg: repeats are the parent's, so one timed pass behind the warming one
        cache_metric = ExtendedDistanceMetric.from_name(args.cache_metric)
        out.update({"storage": "dense", "no_coalesce": bool(os.environ.get("NMN_HNSW_NO_COALESCE")), "caller_calls": args.caller_calls,
                    "cache_metric": cache_metric.name, "k": 1, "threshold": 0.9})
        args.repeats = 1
        with build_or_load(args.index_file, n, d, cfg, "dense", out) as g:
            out.update(time_callers(g, Q, [int(x) for x in args.cache_callers.split(",")], args, cache=cache_metric))
        print(json.dumps(out), flush=True)
        return
    if args.sparse_callers:  # one leg: repeats are the parent's, so one timed pass behind the warming one
        out.update({"storage": args.storage, "no_coalesce": bool(os.environ.get("NMN_HNSW_NO_COALESCE")), "caller_calls": args.caller_calls,
                    "sparse_fraction": args.sparse_fraction})
        del out["k"]
        Qs = Q.copy()
        Qs[np.random.default_rng(0x5BA).random(Qs.shape) < args.sparse_fraction] = 0.0
        args.repeats = 1
        with build_or_load(args.index_file, n, d, cfg, args.storage, out) as g:
            csr = g.sparse_from_dense(Qs)
            per_query = [(np.array([0, int(csr[0][i + 1] - csr[0][i])], np.uint64), csr[1][int(csr[0][i]):int(csr[0][i + 1])],
                          csr[2][int(csr[0][i]):int(csr[0][i + 1])]) for i in range(len(Qs))]
            out["entries_per_query"] = round(float(csr[1].size) / len(Qs), 1)
            out.update(time_callers(g, Qs, [int(x) for x in args.sparse_callers.split(",")], args, sparse=per_query))
        print(json.dumps(out), flush=True)
        return
    if args.sparse_node_fraction is not None:
        print(json.dumps(time_mixed(n, d, cfg, Q, k, args, out)), flush=True)
        return
    if args.tt_node_fraction is not None:
        print(json.dumps(time_tt_nodes(n, d, cfg, k, args, out)), flush=True)
        return
    if args.tt_queries is not None:
        out["storage"] = args.storage
        with build_or_load(args.index_file, n, d, cfg, args.storage, out) as g:
            out.update(time_tt(g, k, args))
        print(json.dumps(out), flush=True)
        return
    if args.sparse_device:
        out["storage"] = args.storage
        with build_or_load(args.index_file, n, d, cfg, args.storage, out) as g:
            out.update(time_sparse_device(g, Q, k, args))
        print(json.dumps(out), flush=True)
        return
    if args.sparse_queries is not None:
        out["storage"] = args.storage
        with build_or_load(args.index_file, n, d, cfg, args.storage, out) as g:
            out.update(time_sparse(g, Q, k, args))
        print(json.dumps(out), flush=True)
        return
    if args.storage == "quantized":
        out["storage"] = "quantized"
        dense_file = args.index_file + ".dense" if args.index_file else None
        with build_or_load(args.index_file, n, d, cfg, "quantized", out, "q8") as gq, build_or_load(dense_file, n, d, cfg, "dense", out, "dense") as gd:
            for name, g in (("q8", gq), ("dense", gd)):
                out[f"{name}_hbm_bytes"], out[f"{name}_max_layer"] = g.hbm_bytes, g.max_layer
            s = torch.cuda.Stream()
            out.update(time_storage(gq, gd, Q, torch.from_numpy(Q).cuda(), k, s, args, metric))
        print(json.dumps(out), flush=True)
        return
    if args.storage == "binary":  # the binary handle is built every run (no file form); --index-file names the DENSE handle's file
        out.update({"storage": "binary", "binary_threshold": args.binary_threshold})
        with build_or_load(None, n, d, cfg, "binary", out, "bin", args.binary_threshold) as gb, \
                build_or_load(args.index_file, n, d, cfg, "dense", out, "dense") as gd:
            for name, g in (("bin", gb), ("dense", gd)):
                out[f"{name}_hbm_bytes"], out[f"{name}_max_layer"] = g.hbm_bytes, g.max_layer
            s = torch.cuda.Stream()
            out.update(time_storage(gb, gd, Q, torch.from_numpy(Q).cuda(), k, s, args, metric, "bin"))
        print(json.dumps(out), flush=True)
        return
    with build_or_load(args.index_file, n, d, cfg, "dense", out) as g:
        out["max_layer"], out["hbm_bytes"] = g.max_layer, g.hbm_bytes
        flat = g.vectors()
        s = torch.cuda.Stream()
        qd = torch.from_numpy(Q).cuda()
        if xmetric is not None:
            out["xmetric"] = xmetric.name
        if args.launch_calls is not None:
            with torch.cuda.stream(s):
                for _ in range(args.launch_calls):
                    if xmetric is not None:
                        g.search_metric_device(qd[:64], k, xmetric, stream=s)
                    else:
                        g.search_device(qd[:64], k, 50, stream=s)
            s.synchronize()
            out["device_calls"] = args.launch_calls
            print(json.dumps(out), flush=True)
            return
        if xmetric is not None:
            out.update(time_rerank(g, xmetric, Q, qd, k, s, args))
            print(json.dumps(out), flush=True)
            return
        for ef in (50, 200):
            r = {}
            # warm every shape, and the three paths against each other
            dev = {}
            for nq in (1, 64, 1024):
                o = (torch.empty((nq, k), dtype=torch.int64, device="cuda"), torch.empty((nq, k), dtype=torch.float32, device="cuda"),
                     torch.empty((nq,), dtype=torch.int32, device="cuda"))
                dev[nq] = o
                g.search_device(qd[:nq], k, ef, out=o, stream=s)
                g.search(Q[:nq], k, ef)
                flat.search(Q[:nq], k, metric)
            s.synchronize()
            ids, sc, cnt, st = g.search(Q, k, ef, with_stats=True)
            r["evals_per_query"] = round(st.rows_scanned / 1024, 1)
            r["spilled_queries"] = int(st.fallback_queries)
            same = np.array_equal(dev[1024][0].cpu().numpy().view(np.uint64), ids) and \
                np.array_equal(dev[1024][1].cpu().numpy().view(np.uint32), sc.view(np.uint32))
            os.environ["NMN_HNSW_HOST_SEARCH"] = "1"
            try:
                t0 = time.perf_counter()
                hids, hsc, _ = g.search(Q[:64], k, ef)
                r["host_ms_per_query"] = round((time.perf_counter() - t0) * 1e3 / 64, 4)
            finally:
                del os.environ["NMN_HNSW_HOST_SEARCH"]
            same = same and np.array_equal(hids, ids[:64]) and np.array_equal(hsc.view(np.uint32), sc[:64].view(np.uint32))
            r["device_host_buffer_and_host_walk_agree"] = bool(same)
            ex_rows, _, _ = flat.search(Q, k, metric)
            r["recall_at_10"] = round(float(np.mean([len(set(a.tolist()) & set(b.tolist())) / k for a, b in zip(ids, ex_rows)])), 4)
            reps = {}
            for _ in range(args.repeats):
                m = {}
                for nq, calls in ((1, args.calls), (64, args.calls), (1024, max(args.calls // 5, 5))):
                    qs = Q[:nq]
                    # the walk and the exhaustive search alternate call by call: both see the same machine state
                    tw, tf = [], []
                    for _ in range(calls):
                        t0 = time.perf_counter()
                        g.search(qs, k, ef)
                        t1 = time.perf_counter()
                        flat.search(qs, k, metric)
                        t2 = time.perf_counter()
                        tw.append(t1 - t0)
                        tf.append(t2 - t1)
                    name = "nq1" if nq == 1 else f"per_query_nq{nq}"
                    m[f"gpu_ms_{name}"] = float(np.median(tw)) * 1e3 / nq
                    m[f"flat_ms_{name}"] = float(np.median(tf)) * 1e3 / nq
                    if nq > 1:
                        ev = []
                        for _ in range(calls):
                            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                            e0.record(s)
                            g.search_device(qd[:nq], k, ef, out=dev[nq], stream=s)
                            e1.record(s)
                            ev.append((e0, e1))
                        s.synchronize()
                        m[f"dev_ms_{name}"] = float(np.median([a.elapsed_time(b) for a, b in ev])) / nq
                t0 = time.perf_counter()
                for _ in range(args.b2b):
                    g.search_device(qd[:64], k, ef, out=dev[64], stream=s)
                s.synchronize()
                m["b2b_ms_per_query_nq64"] = (time.perf_counter() - t0) * 1e3 / args.b2b / 64
                for key, v in m.items():
                    reps.setdefault(key, []).append(v)
            for key, v in reps.items():
                r[key] = round(float(np.median(v)), 5)
                r[key + "_spread"] = round(float((max(v) - min(v)) / np.median(v)), 3)
            out[f"ef{ef}"] = r
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
