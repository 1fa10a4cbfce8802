"""Runs the forced cases of tests/_select_walk_cases.py on the GPU, one after another, and prints one JSON line per case.

The parent (tests/test_gpu_select_walk.py) starts ONE of these per run of the module, with NMN_NO_FLAT_SELECT=1 in the child's
environment: the switch is read once per process.  The first HIP error or failed call ends the run: nothing is started after it,
the cases that were not reached have no line and fail in the parent with this process's last output.

    NMN_NO_FLAT_SELECT=1 python -m tests._select_walk_worker [case id ...]"""
import json
import sys
import time

import numpy as np

from tests import _select_walk_cases as sw


def load_index(case, corpus):
    """A shard holding corpus.A, the mirror mode set BEFORE the rows arrive (mode 0 then builds no mirror: the f32 matrix-core
    sweep's margin is the a-priori one, as in tests/test_gpu_margin_attack.py)."""
    from neumann_amd import GpuFlatIndex
    n, d = corpus.A.shape
    idx = GpuFlatIndex(d, n, single_launch=False, cand_cap=case.cand_cap)
    idx.set_mirror(case.mode)
    if corpus.synthetic is not None:
        seed, rows = corpus.synthetic
        idx.fill_synthetic(seed, n)
        for r in rows:
            idx.set_row(int(r), corpus.A[r])
    else:
        idx.upload(corpus.A)
    return idx


def index_key(case):
    fresh_per_mode = case.corpus[0] in ("attack", "crowd_attack")
    return (case.corpus, case.cand_cap, case.mode if fresh_per_mode else None)


def run_case(idx, case, corpus):
    from neumann_amd import _capi
    geo = sw.case_geometry(case, *corpus.A.shape)
    Q = sw.build_queries(case, corpus)
    mask = sw.build_mask(case, corpus, geo)
    idx.set_mirror(case.mode)
    before = _capi.select_form_counts()
    t0 = time.perf_counter()
    rows, scores, counts, st = idx.search(Q, case.k, case.metric, mask=mask, with_stats=True)
    dt = time.perf_counter() - t0
    after = _capi.select_form_counts()
    return dict(id=case.id, rows=[[int(x) for x in r] for r in rows],
                score_bits=[[int(x) for x in r] for r in np.ascontiguousarray(scores, np.float32).view(np.uint32)],
                counts=[int(c) for c in counts],
                stats=dict(sweep=st.sweep, fallback_queries=int(st.fallback_queries), candidates_rescored=int(st.candidates_rescored),
                           sweep_launches=int(st.sweep_launches), rows_scanned=int(st.rows_scanned), bytes_scanned=int(st.bytes_scanned)),
                forms_before=list(before), forms_after=list(after), search_seconds=round(dt, 4))


def main(argv):
    cases = sw.forced_cases()
    if argv:
        cases = [c for c in cases if c.id in set(argv)]
    t_start = time.perf_counter()
    idx, key = None, None
    status, shards = 0, 0
    try:
        for case in cases:
            corpus = sw.build_corpus(case.corpus)
            if index_key(case) != key:
                if idx is not None:
                    idx.close()
                    idx = None
                idx, key = load_index(case, corpus), index_key(case)
                shards += 1
            try:
                line = run_case(idx, case, corpus)
            except Exception as e:  # a failed call (NeumannGpuError carries the HIP error): stop here, run nothing after it
                print(json.dumps(dict(id=case.id, error=f"{type(e).__name__}: {e}")), flush=True)
                status = 1
                break
            print(json.dumps(line), flush=True)
    finally:
        if idx is not None and status == 0:
            idx.close()
    print(json.dumps(dict(worker_seconds=round(time.perf_counter() - t_start, 2), cases=len(cases), shards=shards)), flush=True)
    return status


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
