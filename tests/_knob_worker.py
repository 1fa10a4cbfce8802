"""Runs ONE profile of tests/_knob_cases.py on the GPU, its cases one after another, and prints one JSON line per case.

The parent (tests/test_gpu_knobs.py) starts one of these per profile, strictly one after another, with the profile's switches in
the CHILD's environment: nearly every switch is read once per process.  The first HIP error or failed call ends the run: nothing is
started after it, the cases that were not reached have no line and fail in the parent with this process's last output.

    NMN_NO_MFMA=1 NMN_NO_WALK=1 python -m tests._knob_worker valu [case id ...]

The worker does not set the profile's environment itself — but it refuses to run when its environment does not hold exactly the
profile's NMN_* names and values (a line {"env_mismatch": ...}, exit 2): the environment IS the evidence for the knobs no counter shows."""
import json
import os
import sys
import threading
import time

import numpy as np

from tests import _knob_cases as kc


def _bits(scores):
    return [[int(x) for x in r] for r in np.ascontiguousarray(scores, np.float32).view(np.uint32).reshape(len(scores), -1)]


def _rows(rows):
    return [[int(x) for x in r] for r in np.asarray(rows, np.uint64).reshape(len(rows), -1)]


def _stats(st):
    return dict(sweep=st.sweep, fallback_queries=int(st.fallback_queries), candidates_rescored=int(st.candidates_rescored),
                sweep_launches=int(st.sweep_launches), rows_scanned=int(st.rows_scanned), bytes_scanned=int(st.bytes_scanned))


class Shards:
    """One flat shard at a time, keyed by what a rebuild depends on; the mirror mode is set BEFORE the rows arrive."""

    def __init__(self):
        self.key, self.idx, self.built = None, None, 0

    def get(self, case, corpus):
        from neumann_amd import GpuFlatIndex
        key = (case.corpus, case.cand_cap, case.mode, case.single_launch)
        if key != self.key:
            self.close()
            n, d = corpus.A.shape
            idx = GpuFlatIndex(d, n, single_launch=case.single_launch, cand_cap=case.cand_cap)
            idx.set_mirror(case.mode)
            if corpus.synthetic is not None:
                seed, rows = corpus.synthetic
                idx.fill_synthetic(seed, n)
                for r in rows:
                    idx.set_row(int(r), corpus.A[r])
            else:
                idx.upload(corpus.A)
            self.key, self.idx = key, idx
            self.built += 1
        return self.idx

    def close(self):
        if self.idx is not None:
            self.idx.close()
        self.key, self.idx = None, None


def run_search(shards, case):
    corpus = kc.build_corpus(case)
    idx = shards.get(case, corpus)
    Q = kc.build_queries(case, corpus)
    mask = kc.build_mask(case, corpus.A.shape[0])
    rows, scores, counts, st = idx.search(Q, case.k, case.metric, mask=mask, with_stats=True)
    return dict(rows=_rows(rows), score_bits=_bits(scores), counts=[int(c) for c in counts], stats=_stats(st))


def _in_threads(n, work):
    """work(t) on n threads released together, three rounds each; the first exception is re-raised here."""
    errs, start = [], threading.Barrier(n)

    def body(t):
        try:
            start.wait()
            for _ in range(3):
                work(t)
        except Exception as e:  # noqa: BLE001
            errs.append(e)

    th = [threading.Thread(target=body, args=(t,)) for t in range(n)]
    for x in th:
        x.start()
    for x in th:
        x.join()
    if errs:
        raise errs[0]


def run_threads(shards, case):
    corpus = kc.build_corpus(case)
    idx = shards.get(case, corpus)
    Q = kc.build_queries(case, corpus)
    out = [None] * case.nq
    before = idx.coalesce_stats()

    def work(t):
        out[t] = idx.search(Q[t:t + 1], case.k, case.metric)

    _in_threads(case.threads, work)
    after = idx.coalesce_stats()
    return dict(rows=_rows([o[0][0] for o in out]), score_bits=_bits([o[1][0] for o in out]), counts=[int(o[2][0]) for o in out], stats=None,
                aux=dict(merged_batches=after[0] - before[0], merged_calls=after[1] - before[1]))


def _pred_ops(g, spec, cols):
    code = dict(eq=g.CMP_EQ, lt=g.CMP_LT, ge=g.CMP_GE, gt=g.CMP_GT)
    return [(g.PRED_AND, 0, 0, 0, 0, 0) if op[0] == "and" else (g.PRED_CMP, code[op[0]], g.CELL_INT, cols[op[1]], int(op[2]), 0) for op in spec]


def run_pred(shards, case):
    from neumann_amd import columns as g
    corpus = kc.build_corpus(case)
    idx = shards.get(case, corpus)
    n = corpus.A.shape[0]
    Q = kc.build_queries(case, corpus)
    progs = kc.pred_programs(n, case.nq)
    with g.GpuColumns(n) as gc:
        cols = [gc.add_column(), gc.add_column()]
        for c, values in zip(cols, kc.pred_columns(n)):
            gc.write(c, 0, np.full(n, g.CELL_INT, np.uint8), values.astype(np.uint64))
        gc.write_valid(0, np.full((n + 63) // 64, 0xFFFFFFFFFFFFFFFF, np.uint64))
        out = [None] * case.nq

        def work(j):
            out[j] = idx.search_pred(gc, _pred_ops(g, progs[j][0], cols), [], Q[j], case.k, case.metric)

        if case.threads:
            _in_threads(case.threads, work)
        else:
            for j in range(case.nq):
                work(j)
    return dict(rows=_rows([o[0][0] for o in out]), score_bits=_bits([o[1][0] for o in out]), counts=[int(o[2][0]) for o in out], stats=None,
                aux=dict(selected=[int(o[3]) for o in out]))


def run_engine(case):
    from neumann_amd import engine as E
    A, Q = kc.engine_setup(case.corpus)
    eng = E.VectorEngine()
    try:
        eng.batch_store_embeddings([f"k{i}" for i in range(A.shape[0])], A)
        res = [eng.search_similar(Q[i], case.k) for i in range(case.nq)]
    finally:
        eng.close()
    # (the engine returns the hits only: no padded tail)
    return dict(rows=[[int(r.key[1:]) for r in one] for one in res],
                score_bits=[[int(np.float32(r.score).view(np.uint32)) for r in one] for one in res], counts=[len(one) for one in res], stats=None)


def run_ivf(case):
    from neumann_amd.ivf import GpuIvfFlat
    orc, V, Q = kc.ivf_setup(case.corpus)
    with GpuIvfFlat(orc.centroids, capacity_rows=len(V) + 64, nprobe=orc.nprobe) as gpu:
        gpu.add(V[:1000])
        gpu.add(V[1000:])
        ids, dist, counts = gpu.search(Q[:case.nq], case.k, case.nprobe)
        aux = dict(list_major_rows=gpu.list_major_rows)
    return dict(rows=_rows(ids), score_bits=_bits(dist), counts=[int(c) for c in counts], stats=None, aux=aux)


def run_case(shards, case):
    from neumann_amd import _capi
    before = _capi.select_form_counts()
    t0 = time.perf_counter()
    if case.api == "search":
        line = run_search(shards, case)
    elif case.api == "threads":
        line = run_threads(shards, case)
    elif case.api == "pred":
        line = run_pred(shards, case)
    elif case.api == "engine":
        line = run_engine(case)
    elif case.api == "ivf":
        line = run_ivf(case)
    else:
        raise KeyError(case.api)
    line.update(id=case.id, forms_before=list(before), forms_after=list(_capi.select_form_counts()), case_seconds=round(time.perf_counter() - t0, 4))
    return line


def main(argv):
    prof = kc.PROFILE[argv[0]]
    mine = {k: v for k, v in os.environ.items() if k.startswith("NMN_")}
    if mine != dict(prof.env):
        print(json.dumps(dict(env_mismatch=mine, profile=prof.name)), flush=True)
        return 2
    cases = [kc.CASES[c] for c in prof.cases if len(argv) == 1 or c in argv[1:]]
    t_start = time.perf_counter()
    shards, status = Shards(), 0
    try:
        for case in cases:
            try:
                line = run_case(shards, case)
            except Exception as e:  # a failed call (NeumannGpuError carries the HIP error): stop here, run nothing after it
                print(json.dumps(dict(id=case.id, error=f"{type(e).__name__}: {e}")), flush=True)
                status = 1
                break
            print(json.dumps(line), flush=True)
    finally:
        if status == 0:
            shards.close()
    print(json.dumps(dict(worker_seconds=round(time.perf_counter() - t_start, 2), profile=prof.name, env=mine, cases=len(cases), shards=shards.built)), flush=True)
    return status


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
