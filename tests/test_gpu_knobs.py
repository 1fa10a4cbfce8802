"""Every documented switch and geometry knob (README.md, "Measurement knobs") held to the oracle: no switch changes a bit of an answer.

tests/_knob_cases.py is the table: profiles (an environment, a list of cases), cases, OUT_OF_SCOPE.  Nearly every switch is read once
per process, so each profile runs in a fresh child (tests/_knob_worker.py).  ONE module-scoped fixture starts the children strictly
one after another — at most one child is alive at any time, each a fresh subprocess.run — and after a child that timed out, died by a
signal or reported a failed call no further child is started: every remaining case fails with that child's last output.

Every case of every profile: rows, score BITS and counts equal the oracle's (computed once per case here in the parent and shared by
all profiles — the answer does not depend on the environment, which is the point), the tail is NO_ROW / -inf (IVF distances: +inf;
the engine returns the hits only).  The baseline profiles (empty environment, the same worker) show that the harness itself agrees
with the oracle and supply the stats of Profile.effects: a case where the switch visibly took effect against the baseline —
stats.sweep, sweep_launches, fallback_queries / candidates_rescored, the IVF's list_major_rows, the coalescer's merged calls.

Knobs whose effect NO existing counter shows; their evidence is the child's environment (the worker refuses to run unless its NMN_*
variables are exactly the profile's) plus, for the geometry knobs, the launch arithmetic that tests/test_knob_table_cpu.py checks:
NMN_SCAN_WAVES, NMN_MFMA_WGS, NMN_RING_WGS, NMN_SCAN_WAVES_SMALL (geometry); NMN_SCAN_NT, NMN_MFMA_NO_FOLD, NMN_MFMA_I8_NO_128,
NMN_MFMA_WAVES, NMN_NO_WALK, NMN_I8_TWO_PLANES, NMN_PRED_TICKET, NMN_ENGINE_TIGHT_ROWS, NMN_NO_ZERO_COPY, NMN_NO_POLL,
NMN_HOST_INFLIGHT, NMN_GATHER_US, NMN_IVF_NO_BATCHED_SCANS, NMN_IVF_NO_DIRECT, NMN_FUSED_TAIL, NMN_NO_SHORT_CHAIN, NMN_NO_EXACT_ROWS,
NMN_NO_GRID_SELECT, NMN_SCAN_I8_WGS_PER_CU, NMN_SCAN_WGS_PER_CU, NMN_SAMPLE_REREAD, NMN_SAMPLE_AHEAD_OF_CHAIN
(Profile.by_arithmetic in the table)."""
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest

from tests import _knob_cases as kc
from tests import _select_walk_cases as sw

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAT, SPLIT, WALK = 0, 1, 2
PAIRS = [(p.name, c) for p in kc.PROFILES for c in p.cases]

# Wall time of each child on an MI355X, seconds: three runs of this module, each on a freshly copied tree, the child the only GPU
# process beside this one (which never opens the GPU itself).  The limit of a child is three times the largest of its runs (the
# factor covers a cold tree and a busy machine), as tests/test_gpu_select_walk.py does for its child.
MEASURED = {
    "base-small": (0.6, 0.6, 0.59),
    "base-pipe": (0.5, 0.5, 0.53),
    "base-host": (0.6, 0.5, 0.45),
    "base-ivf": (0.5, 0.5, 0.45),
    "base-18": (0.8, 0.9, 0.8),
    "base-21": (0.6, 0.6, 0.6),
    "geometry-min": (0.5, 0.6, 0.57),
    "mfma-forms": (0.6, 0.6, 0.53),
    "valu": (0.5, 0.5, 0.51),
    "mfma-min-nq": (0.5, 0.6, 0.54),
    "tiny-i8": (0.5, 0.6, 0.52),
    "route-no-i8-mfma": (0.5, 0.6, 0.54),
    "route-masked-half": (0.5, 0.6, 0.51),
    "route-no-i8": (0.5, 0.5, 0.51),
    "pipeline": (0.6, 0.5, 0.55),
    "host-copy": (0.6, 0.5, 0.56),
    "host-sync": (0.6, 0.6, 0.53),
    "host-no-coalesce": (0.5, 0.6, 2.94),
    "host-inflight": (0.5, 0.4, 0.43),
    "ivf-bitmap": (0.4, 0.5, 0.48),
    "ivf-host-scans": (0.4, 0.5, 0.5),
    "fused-tail": (0.8, 0.9, 0.77),
    "long-chain": (0.8, 0.8, 0.77),
    "no-crowd": (0.7, 0.7, 0.67),
    "ring-geometry": (0.5, 0.6, 0.61),
    "no-ring": (0.6, 0.5, 0.49),
    "wgs-per-cu": (0.4, 0.5, 0.4),
    "sample-reread": (0.6, 0.6, 0.75),
    "no-refine": (0.6, 0.7, 0.58),
    "no-sample": (0.6, 0.6, 0.62),
}
# The three host-concurrency children run the SAME two cases (eight threads) in the same worker, and one of their nine runs stalled:
# 2.65 of host-no-coalesce's 2.94 s went into its first case, whose 24 searches take 0.2 s in every other run — same answers,
# same counters; where it stalled is not known (the first batches of eight threads create the shard's extra host slots: streams,
# workspaces, pinned blocks).  Their runs are pooled: the largest of the nine sets the limit of all three.
POOLED = ("base-host", "host-no-coalesce", "host-inflight")
FIRST_RUN_LIMIT = 60.0   # a profile without a measured time yet; a child that merely needs longer is split, not given more


def _limit(name):
    if name not in MEASURED:
        return FIRST_RUN_LIMIT
    runs = [t for n in POOLED for t in MEASURED[n]] if name in POOLED else MEASURED[name]
    return 3.0 * max(runs)


def _run_child(profile):
    env = {k: v for k, v in os.environ.items() if not k.startswith("NMN_")}   # the profile's switches and no others
    env.update(profile.env)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    t0 = time.perf_counter()
    try:
        r = subprocess.run([sys.executable, "-m", "tests._knob_worker", profile.name], env=env, cwd=ROOT, capture_output=True, text=True,
                           timeout=_limit(profile.name))   # MEASURED above: 0.4 .. 0.9 s per child in three runs (one stalled run of 2.94 s), times three
        code, out, err = r.returncode, r.stdout, r.stderr
    except subprocess.TimeoutExpired as e:      # the child is killed; what it printed so far still counts
        as_text = lambda b: b.decode(errors="replace") if isinstance(b, bytes) else (b or "")  # noqa: E731
        code, out, err = "timeout", as_text(e.stdout), as_text(e.stderr)
    wall = time.perf_counter() - t0
    lines, own = {}, None
    for ln in out.splitlines():
        if ln.startswith("{"):
            try:
                rec = json.loads(ln)
            except ValueError:                  # (a line cut short by the kill)
                continue
            if "id" in rec:
                lines[rec["id"]] = rec
            elif "worker_seconds" in rec:
                own = rec
    print(f"knob worker {profile.name}: {wall:.2f} s, exit {code}, its own clock {own and own['worker_seconds']} s, "
          f"{len(lines)} of {len(profile.cases)} cases, {own and own['shards']} shards")
    ok = code == 0 and own is not None and not any("error" in rec for rec in lines.values())
    return dict(lines=lines, ok=ok, code=code, wall=wall, last=(out[-600:] if len(out) < 4000 else "... " + out[-300:], err[-3000:]))


@pytest.fixture(scope="module")
def children():
    """Every profile's child, one after another; the first one that ends badly is the last one started."""
    done, stopped_by = {}, None
    for p in kc.PROFILES:
        if stopped_by is not None:
            break
        done[p.name] = _run_child(p)
        if not done[p.name]["ok"]:
            stopped_by = p.name
    print("knob workers, wall seconds: " + json.dumps({n: round(d["wall"], 2) for n, d in done.items()}))
    return done, stopped_by


@pytest.fixture(scope="module")
def oracle():
    """The oracle's answer for a case, computed once and shared by all profiles."""
    held = {}

    def get(case):
        if case.id not in held:
            held[case.id] = kc.oracle_answer(case)
        return held[case.id]

    return get


def _line(children, profile_name, case_id):
    done, stopped_by = children
    child = done.get(profile_name)
    if child is None:
        bad = done[stopped_by]
        pytest.fail(f"profile {profile_name} was not started: the child of {stopped_by} ended badly (exit {bad['code']})\nstdout: {bad['last'][0]}\nstderr: {bad['last'][1]}")
    rec = child["lines"].get(case_id)
    if rec is None:
        pytest.fail(f"the worker of {profile_name} never reached {case_id}: exit {child['code']}\nstdout: {child['last'][0]}\nstderr: {child['last'][1]}")
    assert "error" not in rec, (rec, child["last"][1])
    return rec


def _check_answer(case, rec, expected):
    tail_bits = 0x7F800000 if case.api == "ivf" else 0xFF800000       # +inf distances / -inf scores
    assert len(rec["counts"]) == len(expected) == case.nq, (case.id, len(rec["counts"]), len(expected))
    for i, (er, eb) in enumerate(expected):
        rows, bits = np.asarray(rec["rows"][i], np.uint64), np.asarray(rec["score_bits"][i], np.uint32)
        c = er.size
        assert rec["counts"][i] == c, (case.id, i, rec["counts"][i], c)
        assert np.array_equal(rows[:c], er), (case.id, i, rows[:c][:12], er[:12])
        assert np.array_equal(bits[:c], eb), (case.id, i, bits[:c][:8], eb[:8])
        if case.api == "engine":
            assert rows.size == c, (case.id, i, "the engine returns the hits only")
        else:
            assert rows.size == bits.size == case.k, (case.id, i, rows.size)
            assert np.all(rows[c:] == kc.NO_ROW) and np.all(bits[c:] == tail_bits), (case.id, i, "tail")
    if case.api == "pred":
        _, keeps = zip(*kc.pred_programs(kc.build_corpus(case).A.shape[0], case.nq))
        assert rec["aux"]["selected"] == [int(k.sum()) for k in keeps], (case.id, rec["aux"]["selected"])


@pytest.mark.parametrize("profile_name,case_id", PAIRS, ids=[f"{p}:{c}" for p, c in PAIRS])
def test_switch_leaves_the_answer_alone(children, oracle, profile_name, case_id):
    case = kc.CASES[case_id]
    rec = _line(children, profile_name, case_id)
    st = rec.get("stats")
    moved = [a - b for a, b in zip(rec["forms_after"], rec["forms_before"])]
    print(f"{profile_name}:{case_id}: stats {st}, forms moved {moved}, aux {rec.get('aux')}, {rec['case_seconds']} s")
    _check_answer(case, rec, oracle(case))
    if case.api == "search" and st["sweep"] not in ("exact", "none") and case.k <= 4096:
        # none of the table's switches is a select switch: the form is launch_select's own choice for the shape (flat up to 16 384
        # tiles, the walk for the batches on the 2^21-row shard), and only that form moved
        form = {"flat": FLAT, "split": SPLIT, "walk": WALK}[sw.expected_form(case.corpus[2], case.nq, case.k)]
        assert moved[form] >= 1 and sum(moved) == moved[form], (case_id, moved, form)


def _matches(want, got, other=None):
    if isinstance(want, tuple):
        op = want[0]
        if op == "prefix":
            return isinstance(got, str) and got.startswith(want[1])
        if op == "ne":
            return got != want[1]
        if op == "ge":
            return got >= want[1]
        if op == "differs":
            return got != other
        raise KeyError(op)
    return got == want


def _field(rec, name):
    if name.startswith("aux."):
        return rec["aux"][name[4:]]
    return rec["stats"][name]


EFFECTS = [(p.name, e) for p in kc.KNOB_PROFILES for e in p.effects]


@pytest.mark.parametrize("profile_name,effect", EFFECTS, ids=[f"{p}:{e[0]}:{e[1]}" for p, e in EFFECTS])
def test_switch_took_effect(children, profile_name, effect):
    """The counters that can show a switch at work, against the same case of the baseline profile."""
    case_id, name, base_want, knob_want = effect
    base = _field(_line(children, kc.PROFILE[profile_name].base, case_id), name)
    got = _field(_line(children, profile_name, case_id), name)
    print(f"{profile_name}:{case_id}: {name} baseline {base!r}, under the profile {got!r}")
    assert _matches(base_want, base), (profile_name, case_id, name, "baseline", base, base_want)
    assert _matches(knob_want, got, base), (profile_name, case_id, name, got, knob_want, "baseline", base)


GEOMETRY = [(p.name, c, knob) for p in kc.KNOB_PROFILES for c in p.cases for knob, _, _ in kc.CASES[c].geom if knob in p.env]


@pytest.mark.parametrize("profile_name,case_id,knob", GEOMETRY, ids=[f"{p}:{c}:{k}" for p, c, k in GEOMETRY])
def test_geometry_case_ran_the_sweep_its_claim_is_about(children, profile_name, case_id, knob):
    """The launch arithmetic of a geometry case (tests/test_knob_table_cpu.py) is about one sweep family: that family served."""
    rec = _line(children, profile_name, case_id)
    family = kc.CASES[case_id].family
    assert rec["stats"]["sweep"].startswith(family), (profile_name, case_id, knob, rec["stats"]["sweep"], family)


def test_every_child_ran_every_case_of_its_profile(children):
    done, stopped_by = children
    assert stopped_by is None, (stopped_by, done[stopped_by]["code"], done[stopped_by]["last"])
    for p in kc.PROFILES:
        assert done[p.name]["ok"], (p.name, done[p.name]["last"])
        assert set(done[p.name]["lines"]) == set(p.cases), (p.name, sorted(set(p.cases) - set(done[p.name]["lines"])))
