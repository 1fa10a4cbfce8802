"""tests/_call_circuit.py without a GPU: the call order covers every ordered pair of kinds exactly once, the three palettes build,
every kind's expected answer has the shape its k and bitmap imply, the planted blocks of a palette do not overlap."""
import numpy as np
import pytest

from tests import _call_circuit as cc


@pytest.mark.parametrize("K", [1, 2, 3, 8, 20])
def test_circuit_visits_every_ordered_pair_exactly_once(K):
    c = cc.circuit(K)
    assert len(c) == K * K + 1 and c[0] == c[-1] and set(c) == set(range(K))
    pairs = list(zip(c[:-1], c[1:]))
    assert len(set(pairs)) == len(pairs) == K * K
    assert set(pairs) == {(a, b) for a in range(K) for b in range(K)}
    assert c == cc.circuit(K)      # no randomness


@pytest.mark.parametrize("name", ["L", "T", "S"])
def test_palette_builds_and_its_expected_answers_have_the_implied_shape(name):
    pal = cc.palette(name)
    assert pal.A.shape == (pal.n, pal.d) and pal.A.dtype == np.float32
    assert len(pal.kinds) >= 8
    for kd in pal.kinds:
        assert kd.Q.ndim == 2 and kd.Q.shape[1] == pal.d and kd.metric in (0, 1, 2) and kd.mirror in (0, 1, 2), kd.name
        assert cc.expected_shape_problems(pal, kd) == [], kd.name
        assert (kd.fp is None) == (kd.op == "count"), kd.name       # only count_exact reports no statistics
        if kd.op == "pred":
            assert pal.tag is not None and kd.keep is not None and cc.pred_program(kd, 0), kd.name
        if kd.op != "count":
            assert cc.mismatch(kd, kd.expected) is None, kd.name
    assert {kd.metric for kd in pal.kinds} == {0, 1, 2}
    assert cc.palette(name) is pal     # built once, shared


def test_mismatch_sees_one_wrong_slot_of_any_kind():
    """The comparison the GPU circuits rely on: one row, one score BIT, one count, one stale slot in the padded tail, an unwritten
    count (the device circuit's poison) — each is reported; a -0.0 for a 0.0 too (bits, not values)."""
    kd = cc.palette("S").kind("bitmap_3_rows")          # count 3 < k = 5: two padded slots
    rows, scores, counts = kd.expected

    def changed(which, index, value):
        got = [rows.copy(), scores.copy(), counts.copy()]
        got[which][index] = value
        return cc.mismatch(kd, tuple(got))
    assert cc.mismatch(kd, (rows.copy(), scores.copy(), counts.copy())) is None
    assert "rows differ" in changed(0, (0, 1), rows[0, 0])
    assert "score bits" in changed(1, (0, 2), np.nextafter(scores[0, 2], np.float32(np.inf)))
    assert "counts" in changed(2, 0, 9)
    assert "tail" in changed(0, (0, 4), np.uint64(0xABABABABABABABAB)) and "tail" in changed(1, (0, 3), np.float32(7.0))
    z = cc.Kind("zero", "search", 1, kd.Q, 1, 0)
    z.expected = (np.zeros((1, 1), np.uint64), np.zeros((1, 1), np.float32), np.ones(1, np.uint32))
    assert "score bits" in cc.mismatch(z, (z.expected[0], -z.expected[1], z.expected[2]))
    cnt = cc.palette("T").kind("count_exact")
    assert cc.mismatch(cnt, cnt.expected) is None and cc.mismatch(cnt, (cnt.expected[0] + 1, cnt.expected[1])) is not None


def test_palette_L_names_the_paths_the_issue_lists():
    pal = cc.palette("L")
    sweeps = {kd.fp[0] for kd in pal.kinds if kd.fp}
    assert {"ring_f32", "valu_f32", "valu_bf16", "valu_i8", "mfma_f32", "mfma_bf16", "mfma_i8", "exact"} <= sweeps
    assert int(pal.kind("sparse_bitmap").keep.sum()) < pal.kind("sparse_bitmap").k
    assert 0.38 < pal.kind("pred_40pct").keep.mean() < 0.42 and 15 <= int(pal.kind("pred_few_rows").keep.sum()) <= 45
    # the crowd's copies tie at the top of the crowd query; the near rows fill the top of theirs
    r, s, _ = pal.kind("crowd").expected
    assert np.all((r[0] >= 40_000) & (r[0] < 60_000)) and np.all(s[0] == s[0, 0])
    r, _, _ = pal.kind("near_bf16").expected
    assert np.all((r[0] >= 150_000) & (r[0] < 156_000))
    a, b = pal.kind("near_bf16").Q[0], pal.blocks[1][2].astype(np.float64)
    cos = b @ a / (np.linalg.norm(b, axis=1) * np.linalg.norm(a.astype(np.float64)))
    assert np.percentile(cos, 97.5) - np.percentile(cos, 2.5) < 1e-3 and cos.min() > 0.99
    # the graded block: more than an eighth of the shard (the crowd kernels decline), all of it within 1.8e-3 of the 50th best
    # cosine (inside any bf16 margin: 2 rho_v >= 2.2e-3), fewer rows than the candidate capacity within the f32 margin
    # 2 * 3(d+10)u = 9.5e-5 of it, even at 1.4 times that margin
    a, b = pal.kind("retry_f32").Q[0], pal.blocks[2][2].astype(np.float64)
    cos = b @ a / (np.linalg.norm(b, axis=1) * np.linalg.norm(a.astype(np.float64)))
    c50 = np.sort(cos)[-50]
    assert b.shape[0] * 8 > pal.n and c50 - cos.min() < 1.8e-3
    assert 50 < int(np.sum(cos >= c50 - 6 * (pal.d + 10) * 2.0 ** -24)) < int(np.sum(cos >= c50 - 1.4 * 6 * (pal.d + 10) * 2.0 ** -24)) < 4096
    r, _, _ = pal.kind("retry_f32").expected
    assert np.all((r[0] >= 200_000) & (r[0] < 236_000))


def test_quiet_kinds_and_where_the_full_host_circuits_leave_the_short_chain():
    """The figures tests/test_gpu_call_history.py quotes for its cut: which kinds a host call is flagged for, and the call at which
    the full host circuit of L and of T is flagged first (from there on the host API enqueues the whole chain for 256 calls)."""
    L, T, S = (cc.palette(n) for n in "LTS")
    assert [kd.name for kd in L.kinds if kd.flags] == ["crowd", "near_bf16", "retry_f32", "k4096"] and len(L.quiet_kinds()) == 14
    assert [kd.name for kd in T.quiet_kinds()] == ["bitmap_1pct", "k6000_select_then_sort", "k_all_rows", "count_exact"]
    assert S.quiet_kinds() == S.kinds
    for pal, first in ((L, 18), (T, 0)):
        order = cc.circuit(len(pal.kinds))
        assert next(i for i, ki in enumerate(order) if pal.kinds[ki].flags) == first
        assert len(order) - first > 256 or pal is T       # L: the rule stays in force for most of the circuit
    # a flagged kind shows it in its fingerprint (fallback, crowd list) or is the one kind built for the f32 retry
    for pal in (L, T):
        for kd in pal.kinds:
            if kd.fp is not None:
                assert kd.flags == (kd.fp[2] > 0 or kd.crowd_min > 0 or kd.fits), kd.name


@pytest.mark.parametrize("name", ["L", "T", "S"])
def test_planted_blocks_do_not_overlap(name):
    pal = cc.palette(name)
    spans = sorted((row0, row0 + rows.shape[0]) for _, row0, rows in pal.blocks)
    for (a0, a1), (b0, b1) in zip(spans, spans[1:]):
        assert a1 <= b0, (a0, a1, b0, b1)
    for _, row0, rows in pal.blocks:
        assert 0 <= row0 and row0 + rows.shape[0] <= pal.n and np.array_equal(pal.A[row0:row0 + rows.shape[0]], rows)
