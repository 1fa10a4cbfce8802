"""select_kernel's three-level walk (wave maxima -> tile maxima -> row scores) at its edges, against the oracle.

Since the flat path (shards of <= 16 384 tiles) every small test of the suite selects without the walk; the walk serves the
batched calls on large shards, every k > 256 there and every call with an extra rank.  The cases of tests/_select_walk_cases.py
bring it back to small shards — wave borders, the uint4 tail of the dense gather, partial last waves, ties at a level's k-th
key, fewer valid waves than k, crowds beyond the list caps, the strided tile numbering, the margin attacks, the underflow edge —
with the documented switch NMN_NO_FLAT_SELECT=1, which is read once per process: the FORCED cases run in one child process
(tests/_select_walk_worker.py) per run of this module, the NATURAL ones (shards just over 16 384 tiles, no switch) here.

Every case: rows, score bits and counts equal the oracle's, the tail is NO_ROW / -inf, the form counters
(nmn_select_form_counts) say that the walk — and only the walk — selected, the sweep is the one the case names, and
fallback_queries / candidates_rescored are what the case allows."""
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest

from oracle import oracle_c as oc
from tests import _select_walk_cases as sw

pytestmark = pytest.mark.gpu
U64_MAX = np.uint64(0xFFFFFFFFFFFFFFFF)
FORCED = sw.forced_cases()
NATURAL = sw.natural_cases()
FLAT, SPLIT, WALK = 0, 1, 2
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def forced_lines():
    """The forced cases, run once in one fresh child process with the switch in ITS environment."""
    env = dict(os.environ)
    env["NMN_NO_FLAT_SELECT"] = "1"
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    # the child measured 2.0 s of wall time on an MI355X at most (seven runs of this module, each the first GPU process on a freshly
    # copied tree: 2.0, 2.0, 2.0, 2.0, 1.7, 1.6, 1.8 s; the worker's own `worker_seconds` line, which leaves out the interpreter's
    # start and the imports: 1.48, 1.45, 1.39, 1.51 s).  82 cases, 37 shards built, library load and workspace growth included.  Three times 2.0:
    t0 = time.perf_counter()
    try:
        r = subprocess.run([sys.executable, "-m", "tests._select_walk_worker"], env=env, cwd=ROOT, capture_output=True, text=True, timeout=6.0)
        code, out, err = r.returncode, r.stdout, r.stderr
    except subprocess.TimeoutExpired as e:      # the child is killed; what it printed so far still counts
        as_text = lambda b: b.decode(errors="replace") if isinstance(b, bytes) else (b or "")  # noqa: E731
        code, out, err = "timeout", as_text(e.stdout), as_text(e.stderr)
    print(f"select-walk worker: {time.perf_counter() - t0:.1f} s, exit {code}")
    lines = {}
    for ln in out.splitlines():
        if ln.startswith("{"):
            try:
                rec = json.loads(ln)
            except ValueError:                  # (a line cut short by the kill)
                continue
            if "id" in rec:
                lines[rec["id"]] = rec
            elif "worker_seconds" in rec:
                print(f"select-walk worker, its own clock: {rec['worker_seconds']} s, {rec.get('cases')} cases, {rec.get('shards')} shards")
    return lines, (code, out[-600:] if len(out) < 4000 else "... " + out[-300:], err[-3000:])


def _child_left_the_gpu_usable(forced):
    """False when the child hung, was killed by a signal (abort, segmentation fault, a time limit) or met a failed call (a HIP
    error): nothing more is started on the GPU by this module then."""
    lines, (code, _, _) = forced
    return code == 0 and not any("error" in rec for rec in lines.values())


def _check_answer(case, corpus, Q, mask, rows, bits, counts):
    rows, bits, counts = np.asarray(rows, np.uint64), np.asarray(bits, np.uint32), np.asarray(counts)
    for i in range(Q.shape[0]):
        er, es = oc.search(corpus.A, Q[i], case.k, case.metric, mask=mask, nthreads=8, partial=True, native=True)
        c = er.size
        assert counts[i] == c, (case.id, i, int(counts[i]), c)
        assert np.array_equal(rows[i, :c], er), (case.id, i, rows[i, :c][:12], er[:12])
        assert np.array_equal(bits[i, :c], es.view(np.uint32)), (case.id, i, bits[i, :c][:8], es.view(np.uint32)[:8])
        assert np.all(rows[i, c:] == U64_MAX) and np.all(np.isneginf(bits[i, c:].view(np.float32))), (case.id, i, "tail")


def _check_stats(case, st, before, after):
    moved = [a - b for a, b in zip(after, before)]
    print(f"{case.id}: sweep {st['sweep']}, forms moved {moved}, candidates {st['candidates_rescored']}, fallback {st['fallback_queries']}")
    if case.form == "walk":
        # one launch selects for all queries of a pass, and every case here is ONE pass: a pass takes up to the workspace's query
        # capacity, which is at least 64, the largest nq of a case
        assert moved[WALK] >= 1 and moved[FLAT] == 0 and moved[SPLIT] == 0, (case.id, moved)
    else:
        assert moved[SPLIT] >= 1 and moved[WALK] == 0 and moved[FLAT] == 0, (case.id, moved)
    assert st["sweep"] == case.sweep, (case.id, st["sweep"], case.sweep)
    lo, hi = case.fallback
    assert lo <= st["fallback_queries"] <= hi, (case.id, st["fallback_queries"], case.fallback)
    if case.rescored_max is not None:
        assert st["candidates_rescored"] <= case.rescored_max, (case.id, st["candidates_rescored"], case.rescored_max)
    if case.rescored_min is not None:
        assert st["candidates_rescored"] >= case.rescored_min, (case.id, st["candidates_rescored"], case.rescored_min)


@pytest.mark.parametrize("case", FORCED, ids=[c.id for c in FORCED])
def test_forced_walk_matches_oracle(forced_lines, case):
    lines, last = forced_lines
    rec = lines.get(case.id)
    if rec is None:
        pytest.fail(f"the worker never reached {case.id}: exit {last[0]}\nstdout: {last[1]}\nstderr: {last[2]}")
    assert "error" not in rec, (rec, last[2])
    corpus = sw.build_corpus(case.corpus)
    geo = sw.case_geometry(case, *corpus.A.shape)
    Q = sw.build_queries(case, corpus)
    mask = sw.build_mask(case, corpus, geo)
    _check_answer(case, corpus, Q, mask, rec["rows"], rec["score_bits"], rec["counts"])
    _check_stats(case, rec["stats"], rec["forms_before"], rec["forms_after"])


def test_the_worker_ran_every_case_and_only_walked(forced_lines):
    lines, last = forced_lines
    assert _child_left_the_gpu_usable(forced_lines), last
    assert set(lines) == {c.id for c in FORCED}, last
    recs = [lines[c.id] for c in FORCED]
    assert all(r["forms_after"][FLAT] == 0 and r["forms_after"][SPLIT] == 0 for r in recs), "a forced case left the walk"
    assert recs[-1]["forms_after"][WALK] >= len(FORCED)


@pytest.fixture(scope="module")
def natural_shard(forced_lines):
    """One natural shard at a time (the cases are ordered by shard): synthetic bulk filled on the device, the planted rows set.
    Behind the forced cases' child: after a child that faulted, hung or met a HIP error the natural cases fail here, before any
    GPU call of their own."""
    from neumann_amd import GpuFlatIndex
    if not _child_left_the_gpu_usable(forced_lines):
        pytest.fail(f"the forced cases' child ended badly ({forced_lines[1][0]}): no further GPU work in this module\n{forced_lines[1][2]}")
    held = {}

    def get(key):
        if held.get("key") != key:
            if "idx" in held:
                held.pop("idx").close()
            corpus = sw.build_corpus(key)
            n, d = corpus.A.shape
            idx = GpuFlatIndex(d, n, single_launch=False)
            seed, rows = corpus.synthetic
            idx.fill_synthetic(seed, n)
            for r in rows:
                idx.set_row(int(r), corpus.A[r])
            held.update(key=key, idx=idx, corpus=corpus)
        return held["idx"], held["corpus"]

    yield get
    if "idx" in held:
        held.pop("idx").close()


@pytest.mark.parametrize("case", NATURAL, ids=[c.id for c in NATURAL])
def test_natural_walk_matches_oracle(natural_shard, case):
    """No switch: shards just over 16 384 tiles, where launch_select itself takes the walk (and, for one query at k <= 256, the
    split selection: the k = 256 leg pins the border between the two)."""
    from neumann_amd import _capi
    assert os.environ.get("NMN_NO_FLAT_SELECT") is None and os.environ.get("NMN_NO_SPLIT_SELECT") is None
    idx, corpus = natural_shard(case.corpus)
    geo = sw.case_geometry(case, *corpus.A.shape)
    Q = sw.build_queries(case, corpus)
    mask = sw.build_mask(case, corpus, geo)
    idx.set_mirror(case.mode)
    before = _capi.select_form_counts()
    rows, scores, counts, st = idx.search(Q, case.k, case.metric, mask=mask, with_stats=True)
    after = _capi.select_form_counts()
    assert sw.expected_form(corpus.A.shape[0], case.nq, case.k) == case.form
    _check_answer(case, corpus, Q, mask, rows, np.ascontiguousarray(scores, np.float32).view(np.uint32), counts)
    _check_stats(case, dict(sweep=st.sweep, fallback_queries=int(st.fallback_queries), candidates_rescored=int(st.candidates_rescored)),
                 before, after)
