"""The knob table of tests/_knob_cases.py against the sources and README.md (no GPU):
  * the NMN_* names the sources under neumann_amd/ read are exactly the names of the README's table of measurement knobs;
  * every one of them is set by a profile of tests/test_gpu_knobs.py or has its sentence in OUT_OF_SCOPE;
  * the launch arithmetic of search_enqueue, restated, yields what every geometry case claims."""
import os
import re

import pytest

from tests import _knob_cases as kc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "neumann_amd")
NAME = r"NMN_[A-Z0-9_]+"
# The helpers through which the sources read the environment, listed explicitly: a name is read where one of them is called with
# a string literal.  getenv itself; env_set (nmn_api.hip), env_u32 (nmn_tt.hip) and the lambda `knob` (nmn_scan_ring.hip) wrap it.
READERS = ("getenv", "env_set", "env_u32", "knob")
READ = re.compile(r"\b(?:%s)\(\s*\"(%s)\"" % ("|".join(READERS), NAME))
# ... and the only places where getenv takes something else than a literal: the bodies of those three wrappers
WRAPPER_BODIES = {"csrc/nmn_api.hip": 1, "csrc/nmn_tt.hip": 1, "csrc/nmn_scan_ring.hip": 1}
NOT_ENVIRONMENT = {"NMN_INDEX_WIDE_ROWS"}                  # a flag of nmn_index_desc that the table's text mentions
READ_OUTSIDE_THE_PACKAGE = {"NMN_BENCH_CPU_SAMPLE": "bench.py"}


def _sources():
    for base, _, files in os.walk(SRC):
        for f in sorted(files):
            if f.endswith((".hip", ".cpp", ".h", ".py")):
                path = os.path.join(base, f)
                with open(path, encoding="utf-8") as fh:
                    yield os.path.relpath(path, SRC).replace(os.sep, "/"), fh.read()


def names_read(sources):
    """-> (the names read, the findings that make the scan untrustworthy).  `sources`: (relative path, text) pairs."""
    names, findings = set(), []
    for rel, text in sources:
        names.update(READ.findall(text))
        # a quoted NMN_ name that none of the listed helpers takes: a new spelling of an environment read (or not a read at all:
        # then spell it so that this test can tell)
        for m in re.finditer(r"\"(%s)\"" % NAME, text):
            if not READ.search(text[max(0, m.start() - 40):m.end()]):
                findings.append(f"{rel}: \"{m.group(1)}\" is not an argument of {READERS}")
        # getenv and its kin with a non-literal argument, outside the three wrappers
        loose = len(re.findall(r"\b(?:secure_)?getenv\s*\(\s*(?!\")", text))
        if loose != WRAPPER_BODIES.get(rel, 0):
            findings.append(f"{rel}: {loose} getenv call(s) with a non-literal argument, expected {WRAPPER_BODIES.get(rel, 0)}")
        if rel.endswith(".py") and re.search(r"environ[^\n]*NMN_|getenv[^\n]*NMN_", text):
            findings.append(f"{rel}: reads an NMN_ variable from Python")
    return names, findings


def readme_table_names():
    with open(os.path.join(ROOT, "README.md"), encoding="utf-8") as fh:
        text = fh.read()
    start = text.index("Measurement knobs (environment variables")
    table = text[start:text.index("Reproducing the numbers", start)]
    rows = [ln for ln in table.splitlines() if ln.startswith("| `")]
    assert len(rows) > 40, len(rows)
    return set(re.findall(NAME, "\n".join(rows))) - NOT_ENVIRONMENT


def test_the_scan_finds_every_read_through_the_listed_helpers_only():
    names, findings = names_read(_sources())
    assert not findings, findings
    assert len(names) > 60, sorted(names)
    # the scan itself: a read through a helper it does not know, and a loose getenv, are findings
    _, f = names_read([("csrc/x.hip", 'static bool v = my_env("NMN_X");')])
    assert f and "NMN_X" in f[0]
    _, f = names_read([("csrc/x.hip", "const char* e = getenv(which);")])
    assert f and "non-literal" in f[0]
    n, f = names_read([("csrc/x.hip", 'if (getenv("NMN_X")) return;')])
    assert n == {"NMN_X"} and not f


def test_readme_table_lists_exactly_the_names_the_sources_read():
    read, _ = names_read(_sources())
    for name, where in READ_OUTSIDE_THE_PACKAGE.items():
        with open(os.path.join(ROOT, where), encoding="utf-8") as fh:
            assert re.search(r"environ[^\n]*\"%s\"" % name, fh.read()), (name, where)
    listed = readme_table_names()
    assert read | set(READ_OUTSIDE_THE_PACKAGE) == listed, dict(read_but_not_listed=sorted(read - listed),
                                                                listed_but_not_read=sorted(listed - read - set(READ_OUTSIDE_THE_PACKAGE)))


def test_every_name_is_set_by_a_profile_or_out_of_scope():
    read, _ = names_read(_sources())
    every = read | set(READ_OUTSIDE_THE_PACKAGE)
    by_profile = kc.knobs_set_by_profiles()
    assert by_profile <= every, sorted(by_profile - every)
    assert set(kc.OUT_OF_SCOPE) <= every, sorted(set(kc.OUT_OF_SCOPE) - every)
    assert not by_profile & set(kc.OUT_OF_SCOPE), sorted(by_profile & set(kc.OUT_OF_SCOPE))
    missing = every - by_profile - set(kc.OUT_OF_SCOPE)
    assert not missing, sorted(missing)
    for name, why in kc.OUT_OF_SCOPE.items():
        assert len(why) > 10, name
        m = re.match(r"(tests/\w+\.py)", why)     # "a knob an existing test sets": that test names it
        if m:
            with open(os.path.join(ROOT, m.group(1)), encoding="utf-8") as fh:
                assert name in fh.read(), (name, m.group(1))


def test_profiles_and_cases_are_consistent():
    for p in kc.PROFILES:
        assert p.cases and all(c in kc.CASES for c in p.cases), p.name
        assert len(set(p.cases)) == len(p.cases), p.name
        if p.base is None:
            assert p.env == {} and not p.effects, p.name
            continue
        base = kc.PROFILE[p.base]
        assert base.base is None and set(p.cases) <= set(base.cases), p.name
        assert p.env and p.why, p.name
        # every knob of a profile shows through a counter, or is named as one whose evidence is environment + arithmetic
        assert p.effects or p.by_arithmetic, p.name
        assert set(p.by_arithmetic) <= set(p.env), p.name
        for case_id, name, _, _ in p.effects:
            assert case_id in p.cases, (p.name, case_id)
            assert name in ("sweep", "sweep_launches", "fallback_queries", "candidates_rescored") or name.startswith("aux."), (p.name, name)
    used = {c for p in kc.PROFILES for c in p.cases}
    assert used == set(kc.CASES), sorted(set(kc.CASES) - used)
    assert all(any(c in p.cases for p in kc.KNOB_PROFILES) for c in kc.CASES), "a case that only a baseline runs"


def test_small_cases_cover_the_shapes_the_table_promises():
    small = [c for c in kc.SMALL]
    assert {c.corpus[2] for c in small} == {1, 63, 65, 1000, 4097, 16400, 20011}
    assert {c.corpus[3] for c in small} == {8, 100, 128, 768}
    assert {c.nq for c in small} >= {1, 2, 5, 17, 65}
    assert {c.k for c in small} == {1, 10, 100}
    assert {c.metric for c in small} == {kc.COS, kc.L2, kc.DOT}
    assert {c.mask for c in small} == {None, 0.3, 0.02}
    assert {c.mode for c in small} == {0, 1, 2}
    assert 24 <= len(small) <= 48       # a fixed list of a few dozen, not the product


GEOM = [(c.id, knob, value, claim) for c in kc.ALL_CASES for knob, value, claim in c.geom]


@pytest.mark.parametrize("case_id,knob,value,claim", GEOM, ids=[f"{c}:{k}={v}:{cl}" for c, k, v, cl in GEOM])
def test_geometry_case_yields_what_it_claims(case_id, knob, value, claim):
    case = kc.CASES[case_id]
    rows = case.corpus[2]
    assert kc.claim_holds(claim, rows, value), (case_id, knob, value, claim, kc.launch_arithmetic(rows, value))
    # ... and under the default geometry it does NOT (else the knob adds nothing): 4096 waves / ring groups, 1024 workgroups, 768 small waves
    default = {"NMN_SCAN_WAVES": 4096, "NMN_MFMA_WGS": 1024, "NMN_RING_WGS": 4096, "NMN_SCAN_WAVES_SMALL": 768}[knob]
    if claim == "short_last":
        assert not kc.claim_holds(claim, rows, default) or kc.launch_arithmetic(rows, default)[1] != kc.launch_arithmetic(rows, value)[1]
    # the profile that sets the knob sets it to this value and runs the case
    setters = [p for p in kc.KNOB_PROFILES if p.env.get(knob) == str(value) and case_id in p.cases]
    assert setters, (case_id, knob, value)
    assert case.family in ("valu", "mfma", "ring")
    # the knob's limits as search_enqueue clamps them
    low = {"NMN_SCAN_WAVES": 256, "NMN_MFMA_WGS": 64, "NMN_RING_WGS": 64, "NMN_SCAN_WAVES_SMALL": 256}[knob]
    assert low <= value <= 4096


def test_geometry_knobs_cover_their_claims():
    got = {}
    for _, knob, _, claim in GEOM:
        got.setdefault(knob, set()).add(claim)
    for knob in kc.FULL_CLAIM_KNOBS:
        assert got.get(knob) == set(kc.CLAIMS), (knob, got.get(knob))
    for knob in kc.SHORT_LAST_ONLY_KNOBS:       # (tests/_knob_cases.py says why the other two claims are out of their reach)
        assert got.get(knob) == {"short_last"}, (knob, got.get(knob))
    assert set(got) == set(kc.FULL_CLAIM_KNOBS) | set(kc.SHORT_LAST_ONLY_KNOBS)
    # the reach itself, from the dispatch conditions: the ring sweep needs 4096 tiles, the small-wave band 128 MiB of sweep
    for rows in range(1, 4096 * kc.TILE - 62, 997):
        assert not kc.claim_holds("short_last", rows, 4096)     # below 4096 tiles a 4096-wave grid gives every wave one tile
    case = kc.CASES["b-valu-f32-nq2"]
    assert (128 << 20) <= case.corpus[2] * case.corpus[3] * 4 < (2 << 30) and case.mode == 0 and case.nq <= 2 and case.mask is None
    assert -(-kc.CASES["b-ring-f32"].corpus[2] // kc.TILE) >= 4096
