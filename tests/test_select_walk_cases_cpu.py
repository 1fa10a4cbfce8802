"""The constructions of tests/_select_walk_cases.py, checked without a GPU: the planted rows sit in the tiles and scan waves the
cases claim, tie runs have the stated length and equal score bits in the oracle, crowds exceed the caps they aim at, the gather
a case names is the one its exact scores select (far from the kernel's 0.5), the oracle's answer starts with the planted rows,
and launch_select's own rules predict the form each natural case states."""
import numpy as np
import pytest

from oracle import oracle_c as oc
from tests import _select_walk_cases as sw

FORCED = sw.forced_cases()
NATURAL = sw.natural_cases()
ALL = FORCED + NATURAL
BY_ID = {c.id: c for c in ALL}


def _built(case):
    corpus = sw.build_corpus(case.corpus)
    geo = sw.case_geometry(case, *corpus.A.shape)
    Q = sw.build_queries(case, corpus)
    mask = sw.build_mask(case, corpus, geo)
    return corpus, geo, Q, mask


def test_geometry_restates_search_enqueue():
    """Hand-computed instances of the three rules (tiles per wave: 4096 waves; 768 for unmasked VALU sweeps of 0.125 .. 2 GiB;
    1024 matrix-core workgroups) and of both tile numberings."""
    g = sw.geometry(270_000, 128, "ring_f32", False)
    assert (g.n_tiles, g.tpw, g.W, g.strided) == (4219, 2, 2110, False) and g.tiles_of_wave(2109) == [4218]
    g = sw.geometry(270_000, 128, "mfma_bf16", False)
    assert (g.tpw, g.W) == (5, 844) and g.tiles_of_wave(843) == [4215, 4216, 4217, 4218]
    g = sw.geometry(270_000, 128, "valu_f32", True)
    assert (g.tpw, g.W, g.strided) == (2, 2110, True) and g.tiles_of_wave(5) == [5, 2115] and g.tiles_of_wave(2109) == [2109]
    assert sw.geometry(270_000, 128, "mfma_f32", True).strided is False
    g = sw.geometry(270_000, 256, "valu_f32", False)          # 276 MB of f32 rows: 768 waves
    assert (g.tpw, g.W) == (6, 704)
    assert sw.geometry(270_000, 256, "valu_i8", False).tpw == 2     # 69 MB: 4096 waves
    g = sw.geometry(sw.N_NAT1, 128, "valu_i8", False)            # 134.4 MB >= 128 MiB
    assert (g.n_tiles, g.tpw, g.W) == (16407, 22, 746)
    assert sw.geometry(8193, 256, "mfma_i8", False) == sw.Geometry(129, 1, 129, False)
    assert sw.geometry(sw.N_NAT2, 128, "ring_f32", False).tpw == 8 and sw.geometry(sw.N_NAT2 - 64, 128, "ring_f32", False).tpw == 7
    assert sw.row_stride(128) == 128 and sw.row_stride(300) == 304 and sw.row_stride(120) == 128 and sw.row_stride(24) == 24


def test_forms_follow_the_16384_tile_and_lone_caller_rules():
    for c in FORCED:
        n = c.corpus[2] if c.corpus[0] in ("borders", "plain", "ties") else None
        if n is not None:
            assert sw.expected_form(n, c.nq, c.k) == "flat", c.id       # without the switch these shards never walk
    for c in NATURAL:
        assert sw.expected_form(c.corpus[2], c.nq, c.k) == c.form, c.id
    assert sw.expected_form(sw.FLAT_TILES * 64, 64, 1000) == "flat" and sw.expected_form(sw.FLAT_TILES * 64 + 1, 64, 10) == "walk"
    assert sw.expected_form(sw.N_NAT1, 4, 256) == "split" and sw.expected_form(sw.N_NAT1, 5, 256) == "walk"
    assert {c.form for c in NATURAL} == {"walk", "split"}


def test_the_case_list_covers_what_it_must():
    sweeps = {c.sweep for c in FORCED if c.id.startswith("kind-")}
    assert sweeps == {"ring_f32", "valu_f32", "valu_bf16", "valu_i8", "mfma_f32", "mfma_bf16", "mfma_i8"}
    assert {c.k for c in FORCED} >= {1, 64, 1000, 4096} and {c.nq for c in FORCED} >= {1, 2, 5, 8, 64}
    assert max(c.nq for c in ALL) <= 64, "one query pass per case (a workspace takes at least 64 queries a pass)"
    assert all(c.sweep in sw.ELEM_BYTES and c.fallback[0] == c.fallback[1] for c in ALL), "every case names its sweep and pins fallback_queries"
    assert {c.mode for c in FORCED} == {0, 1, 2} and {c.metric for c in FORCED} == {0, 1, 2}
    assert {c.gather for c in NATURAL} >= {"dense", "quads", "generic"}
    tiles = {sw.geometry(c.corpus[2], c.corpus[3], c.sweep, False).n_tiles % 4 for c in FORCED if c.corpus[0] == "borders"}
    assert tiles >= {1, 3}
    # every construction tests/test_gpu_margin_attack.py runs at its N = 8192, by (construction, metric, arguments, mode, sweep)
    from tests import test_gpu_margin_attack as tma
    want = {(p.values[0], p.values[1], tuple(sorted(p.values[2].items())), p.values[3], p.values[4], p.values[6]) for p in tma._cases()}
    have = {(c.corpus[1], c.corpus[2], c.corpus[3], c.mode, c.sweep, c.mask is not None) for c in FORCED if c.corpus[0] == "attack"}
    assert want == have, want ^ have


@pytest.mark.parametrize("cid", [c.id for c in ALL if c.borders])
def test_planted_rows_sit_where_the_case_says(cid):
    case = BY_ID[cid]
    corpus, geo, Q, mask = _built(case)
    n = corpus.A.shape[0]
    assert {b[0] for b in case.borders} == set(corpus.planted.tolist())
    for row, tile, wave in case.borders:
        assert 0 <= row < n and tile == row // 64 and tile in geo.tiles_of_wave(wave), (row, tile, wave)
    waves = {r: w for r, _, w in case.borders}
    rows = sorted(waves)
    # both ends of the shard, and two neighbouring rows in different scan waves (a wave border)
    assert rows[0] == 0 and 63 in waves and rows[-1] == n - 1
    assert any(b - a == 1 and waves[a] != waves[b] for a, b in zip(rows, rows[1:])), "no wave border among the planted rows"
    if not case.forced:
        a, b = corpus.ties
        assert b - a == 1 and np.array_equal(corpus.A[a], corpus.A[b]), "exact copies across a wave border"
    if cid.startswith("b129"):
        assert geo.n_tiles % 4 == 1 and n % 64 == 1 and geo.tiles_of_wave(geo.W - 1) == [geo.n_tiles - 1], "last wave: one tile, one row"
    if cid.startswith("b139") or cid.startswith("big-"):
        assert geo.n_tiles % 4 == 3 and n % 64 != 0
    if cid in ("big-ring_f32", "big-valu_i8"):
        assert waves[127] == 0 and waves[128] == 1 and geo.tiles_of_wave(geo.W - 1) == [geo.n_tiles - 1] and waves[n - 1] == geo.W - 1
    if cid == "big-mfma_bf16":
        assert waves[319] == 0 and waves[320] == 1 and len(geo.tiles_of_wave(geo.W - 1)) == 4
    if cid == "big-valu_f32-bitmap":
        assert waves[0] == waves[63] == 0 and waves[127] == 1 and waves[n - 1] == (geo.n_tiles - 1) - geo.W   # tile j * W + w
    if mask is not None:
        assert sw.keep_bits(mask, n)[corpus.planted].all()


@pytest.mark.parametrize("cid", [c.id for c in ALL if c.corpus[0] in ("borders", "natural", "ties", "attack", "crowd_attack")
                                 and (c.mask is None or c.mask[0] == "random")])     # (bitmaps that keep the planted rows)
def test_oracle_answer_starts_with_the_planted_rows(cid):
    case = BY_ID[cid]
    corpus, geo, Q, mask = _built(case)
    qi = sw.attack_query_index(case)
    assert np.array_equal(Q[qi], corpus.q)
    p = corpus.planted.size
    er, es = oc.search(corpus.A, Q[qi], max(case.k, p), case.metric, mask=mask, nthreads=8, partial=True, native=True)
    if case.corpus[0] in ("attack", "crowd_attack"):
        assert er[0] == corpus.planted[0], "the target first"
        assert set(er[:case.k].tolist()) <= set(corpus.planted.tolist())
    else:
        assert set(er[:p].tolist()) == set(corpus.planted.tolist())
    if case.tie_len:
        run = es[case.lead:case.lead + case.tie_len].view(np.uint32)
        assert np.all(run == run[0]) and es[case.lead - 1] > es[case.lead], "a run of equal score bits behind the better rows"
        assert np.array_equal(er[case.lead:case.lead + case.tie_len], corpus.ties[:case.tie_len]), "ties in row order"
        full = es[case.lead:p].view(np.uint32)
        assert np.all(full == run[0]) and case.lead + case.tie_len == case.k < p, "the cut falls inside the run"


def test_tie_runs_share_waves_and_tiles_as_stated():
    a, b = sw.build_corpus(sw.TIES_WAVES), sw.build_corpus(sw.TIES_TILE)
    g = sw.geometry(sw.NT, sw.DT, "valu_bf16", False)
    assert g.tpw == 1 and len({g.wave_of_row(r) for r in a.ties}) == a.ties.size == 20 > 10, "a copy per scan wave, more than k"
    assert len({r // 64 for r in b.ties}) == 1 and b.ties.size == 20 > 10, "more than k copies inside one tile"
    for c in (a, b):
        assert all(np.array_equal(c.A[r], c.A[c.ties[0]]) for r in c.ties)


@pytest.mark.parametrize("cid", [c.id for c in FORCED if c.crowd_over])
def test_crowds_exceed_the_caps_they_aim_at(cid):
    case = BY_ID[cid]
    corpus, geo, Q, mask = _built(case)
    what, cap = case.crowd_over
    n = corpus.A.shape[0]
    assert n >= sw.CROWD_MIN_ROWS, "crowd kernels and the f32 retry are present from 2^18 rows"
    if what == "cand_cap" and case.corpus[0] == "crowd_attack":
        assert case.cand_cap == cap and corpus.planted.size == 201 > cap
        v = corpus.info["by_sweep"]["valu_bf16"]
        assert corpus.info["floor"] <= v["sharpness"] < 1.0, "target and decoys are inside the margin, by the model"
    else:
        s = oc.scores_all(corpus.A, Q[0], case.metric, nthreads=8, native=True).view(np.uint32)
        top = s[corpus.ties[0]]
        assert np.all(s[corpus.ties] == top) and float(s.view(np.float32).max()) == float(top.view(np.float32)), "the copies tie at the top"
        tiles = np.unique(corpus.ties // 64).size
        assert tiles > sw.LIST_CAP > sw.BAIL_TILES and corpus.ties.size > sw.CAND_CAP and tiles > cap


@pytest.mark.parametrize("cid", [c.id for c in ALL if c.gather])
def test_the_named_gather_is_the_one_the_scores_select(cid):
    case = BY_ID[cid]
    corpus, geo, Q, mask = _built(case)
    n = corpus.A.shape[0]
    keep = None if mask is None else sw.keep_bits(mask, n)
    for qi in range(Q.shape[0]):
        s = oc.scores_all(corpus.A, Q[qi], case.metric, nthreads=8, native=True)
        share = sw.wave_share(s, geo, case.k, keep)
        assert sw.gather_share_ok(case, share), (cid, qi, share)
        assert sw.gather_kind(geo, share) == case.gather, (cid, qi, share, geo)


@pytest.mark.parametrize("cid", ["few-94-tiles-k100", "few-3-waves-mfma", "few-3-waves-strided", "mask-empty", "mask-7-rows-k10"])
def test_fewer_valid_waves_than_k(cid):
    case = BY_ID[cid]
    corpus, geo, Q, mask = _built(case)
    n = corpus.A.shape[0]
    keep = np.ones(n, bool) if mask is None else sw.keep_bits(mask, n)
    tiles = np.unique(np.flatnonzero(keep) // 64)
    waves = {geo.wave_of_tile(t) for t in tiles}
    if cid == "few-94-tiles-k100":
        assert geo.W == geo.n_tiles == 94 < case.k
    elif cid.startswith("few-3"):
        assert len(waves) == 3 < case.k < tiles.size and keep.sum() > case.k
    elif cid == "mask-empty":
        assert keep.sum() == 0
    else:
        assert 0 < keep.sum() == 7 < case.k


def test_non_finite_scores_are_among_the_top_k():
    case = BY_ID["nonfinite-all-kinds"]
    corpus, geo, Q, mask = _built(case)
    er, es = oc.search(corpus.A, Q[0], case.k, case.metric, mask=mask, nthreads=8, partial=True, native=True)
    assert er.size == 8 < case.k and er[0] == corpus.info["pinf"] and np.isposinf(es[0])
    assert np.isneginf(es).sum() == 1 and np.isnan(es).sum() == 1 and np.isnan(es[-1]) and er[-1] == corpus.info["nan"]
    top = BY_ID["nonfinite-top"]
    er, es = oc.search(corpus.A, Q[0], top.k, top.metric, nthreads=8, partial=True, native=True)
    assert er[0] == corpus.info["pinf"] and np.isposinf(es[0]) and np.isfinite(es[1:]).all()
