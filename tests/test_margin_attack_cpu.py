"""The margin attacks of tests/_margin_attack.py, checked without a GPU: every construction is as sharp as its floor says,
its planted values are exactly the intended ones, the oracle ranks target then decoys, the modelled mirror ranks every decoy
above the target, and the bulk stays out of the way."""
import numpy as np
import pytest

from oracle import oracle_c as oc
from tests import _margin_attack as ma

F = np.float32
IDS = [f"{n}-{'cos l2 dot'.split()[m]}{'-1plane' if kw.get('planes') == 1 else '-2planes' if kw.get('planes') == 2 else ''}" for n, m, kw in ma.CASES]


@pytest.fixture(params=ma.CASES, ids=IDS)
def case(request):
    name, metric, kw = request.param
    return ma.build(name, metric, **kw)


def _off_tie_bf16(x):
    return np.all((x.view(np.uint32) & np.uint32(0xFFFF)) != np.uint32(0x8000))


def _off_tie_i8(t, second_plane):
    """t = x * 127 / max|x|: not half-way between two codes of the first plane, nor (two planes) of the second."""
    ok = np.all(np.abs(t - np.floor(t)) != 0.5)
    if second_plane:
        r = (t - np.rint(t)) * 256.0
        ok = ok and np.all(np.abs(r - np.floor(r)) != 0.5) and np.all(np.abs(np.rint(r)) <= 127)
    return ok


def test_sharpness_reaches_its_floor(case):
    A, q, k, metric, rows, info = case
    for sw, v in info["by_sweep"].items():
        print(f"{info['name']} metric {metric} {sw}: sharpness {v['sharpness']:.4f} (floor {info['floor']}), E {v['E']:.4g}")
        assert info["floor"] <= v["sharpness"] < 1.0, (sw, v["sharpness"])
    if info["name"] == "both_i8":          # the rows' 0.95 times rho_v's share of the claimed sum, from the model
        v = info["by_sweep"]["valu_i8"]
        assert info["floor"] == 0.95 * v["rho_v"] / (v["rho_v"] + v["rho_q"] * (1.0 + v["rho_v"])) and 0.945 < info["floor"] < 0.95
    else:
        assert info["floor"] == (0.95 if info["name"].startswith("rows_") else 0.65)
    assert info["sharpness"] == min(v["sharpness"] for v in info["by_sweep"].values())


def test_planted_values_are_the_intended_ones(case):
    A, q, k, metric, rows, info = case
    assert A.dtype == F and q.dtype == F and k == ma.K and rows.size == 1 + ma.N_DECOYS >= 1 + k
    assert len({int(r) // 64 for r in rows}) == rows.size            # a tile each: the bound is a k-th largest tile maximum
    P, G, B = A[rows], info["G"], info["B"]
    name = info["name"]
    # the error part, element by element, as float64 expressions that must survive the float32 round trip
    if name == "rows_bf16":
        assert np.all(P[0, G].astype(np.float64) == 1 + 2.0 ** -8 - 2.0 ** -16) and np.all(P[1:, G].astype(np.float64) == 1 + 2.0 ** -8 + 2.0 ** -16)
        assert np.all(ma.bf16(P[0, G]) == 1.0) and np.all(ma.bf16(P[1:, G]) == F(1 + 2.0 ** -7))
    elif name in ("rows_i8", "both_i8"):
        assert np.all(P[0, G].astype(np.float64) == 32.5 - 2.0 ** -16) and np.all(P[1:, G].astype(np.float64) == 32.5 + 2.0 ** -16)
        s, c, _ = ma.q8_codes(P)
        assert np.all(s == 1.0) and np.all(c[0, G] == 32) and np.all(c[1:, G] == 33)
    elif name == "query_bf16":
        h = G[: G.size // 2]
        assert np.all(q[h].astype(np.float64) == 1 + 2.0 ** -8 - 2.0 ** -16) and np.all(q[G[G.size // 2:]].astype(np.float64) == 1 + 2.0 ** -8 + 2.0 ** -16)
        assert np.all(P[0, h] == 1) and np.all(P[0, G[G.size // 2:]] == 0) and np.all(P[1:, h] == 0) and np.all(P[1:, G[G.size // 2:]] == 1)
    # no element of a planted row or of the query on a tie of the format it is stored in
    if info["row_format"] == "bf16":
        assert _off_tie_bf16(P) and _off_tie_bf16(q)
        assert np.all(ma.bf16(P[:, B]) == P[:, B]), "B carries no error"
        if info["query_exact"] == "bf16":
            assert np.all(ma.bf16(q) == q)
        else:
            assert np.all(ma.bf16(q[B]) == q[B]) and np.all(ma.bf16(A) == A), "the query attack: every row is exact"
    else:
        s, c, t = ma.q8_codes(P)
        assert np.all(s == 1.0) and _off_tie_i8(t.astype(np.float64), False)
        assert np.all(c[:, B] == P[:, B]), "B carries no error"
        qs, _, qt = ma.q8_codes(q)
        assert qs[0] == 1.0 and _off_tie_i8(qt.astype(np.float64), "mfma_i8_one" not in info["by_sweep"])
        for sw in info["by_sweep"]:
            _, qst = ma.stored(P, q, sw)
            assert np.all(qst[B] == q[B]), "the query's B part is exact in its planes"
            if info["query_exact"] is not None:
                assert np.all(qst == q), sw
            else:
                assert np.any(qst[G] != q[G])
        if info["query_exact"] is None and name == "query_i8":
            assert np.all(ma.q8_rows(A) == A), "the query attack: every row is exact"


def test_oracle_ranks_target_then_decoys(case):
    A, q, k, metric, rows, info = case
    for native in (False, True):
        er, es = oc.search(A, q, rows.size, metric, nthreads=8, partial=True, native=native)
        assert np.array_equal(er, rows.astype(np.uint64)), (er, rows)
        assert np.all(np.diff(es.astype(np.float64)) < 0), "strictly decreasing, no ties"
        assert np.array_equal(es, info["exact_scores"])
    # ... a few distinct f32 scores apart: the whole planted ladder is small against E
    for sw, v in info["by_sweep"].items():
        span = float(es[0]) - float(es[k])
        if v["space"] != "score":
            p = 2.0 if v["space"] == "dist2" else 1.0
            span = (1.0 / float(es[k]) - 1.0) ** p - (1.0 / float(es[0]) - 1.0) ** p
        assert 0 < span < 5e-3 * v["E"], (sw, span, v["E"])


def test_modelled_mirror_ranks_every_decoy_above_the_target(case):
    A, q, k, metric, rows, info = case
    for sw, v in info["by_sweep"].items():
        assert np.all(v["a_decoys"] > v["a_target"]), sw
        assert v["a_k"] - v["a_target"] > 1.25 * v["E"], "a margin of E instead of 2 E would lose the target"
        # the same from the stored corpus itself, searched in float64
        a = ma.model(A, q, metric, sw)["approx"]
        order = np.lexsort((np.arange(a.size), -a))
        assert set(order[:rows.size - 1].tolist()) == set(rows[1:].tolist()) and order[rows.size - 1] == rows[0], sw


def test_bulk_is_out_of_the_way(case):
    A, q, k, metric, rows, info = case
    for sw, v in info["by_sweep"].items():
        assert v["a_k"] - v["best_bulk"] > 4.0 * v["E"], (sw, v["a_k"], v["best_bulk"], v["E"])
        rel_row, abs_row, norm_row = v["worst_rows"]
        # the claimed E is the planted rows' own: the measured maxima the metric's margin reads come from planted rows
        if info["query_exact"] is None and info["name"].startswith("query_"):
            assert v["rho_v"] == 0.0
        elif metric == ma.L2:
            assert abs_row in rows
        else:
            assert rel_row in rows
        if metric == ma.DOT or v["space"] == "dist2":          # ... and the largest magnitude, where the margin reads it
            assert norm_row in rows
        if v["space"] == "dist2":
            assert np.all(v["a_decoys"] < 0), "no decoy's estimated squared distance is clamped at zero"
    exact = oc.scores_all(A, q, metric, nthreads=8)
    bulk = np.ones(A.shape[0], bool)
    bulk[rows] = False
    assert exact[bulk].max() < exact[rows].min()


# ---------------------------------------------------------------------------------------------- attacks that arrive by write
W_IDS = [f"{n}-{'cos l2 dot'.split()[m]}{'-1plane' if kw.get('planes') == 1 else ''}-{sw}" for n, m, kw, sw in ma.WRITTEN_CASES]


@pytest.mark.parametrize("name,metric,kw,sweep", ma.WRITTEN_CASES, ids=W_IDS)
def test_a_stale_margin_loses_the_written_target_and_the_true_one_keeps_it(name, metric, kw, sweep):
    """written_attack: the shard before its planted rows arrive (B) measures smaller maxima than the planted rows need.  With B's
    maxima the target lies OUTSIDE the claimed margin (stale_sharpness > 1: a write that did not raise them loses it), with A's
    own it lies inside (floor <= sharpness < 1) — for all three stale maxima and for the two error maxima alone."""
    B, A, q, k, planted, info = ma.written_attack(name, metric, **kw)
    A0 = ma.build(name, metric, **kw)[0]
    assert A is A0 and B is not A and B.dtype == F and B.shape == A.shape
    v = info["by_sweep"][sweep]
    stale, stale_err = info["stale_sharpness"][sweep], info["stale_err_sharpness"][sweep]
    rho_b, e_b, v_b = info["stale_maxima"][sweep]
    print(f"{name} metric {metric} {sweep}: sharpness {v['sharpness']:.4f}, stale {stale:.3f}, stale errors only {stale_err:.3f}; "
          f"rho_v {rho_b:.4g} -> {v['rho_v']:.4g}, e_abs {e_b:.4g} -> {v['e_abs']:.4g}, max norm {v_b:.4g} -> {v['max_norm']:.4g}")
    assert info["floor"] <= v["sharpness"] < 1.0
    assert stale > 1.0 and stale_err > 1.0
    assert rho_b < v["rho_v"] and e_b < v["e_abs"] and v_b <= v["max_norm"]
    # B is A off the planted rows, and bulk on them: none of them is among B's best, and the bulk's best is where it was
    off = np.ones(A.shape[0], bool)
    off[planted] = False
    assert np.array_equal(B[off], A[off])
    for r in planted:
        nb = int(r) + 1 if int(r) + 1 < A.shape[0] else int(r) - 1
        assert off[nb] and np.array_equal(B[r], A[nb])
    er, _ = oc.search(B, q, planted.size, metric, nthreads=8, partial=True, native=True)
    ea = oc.scores_all(A, q, metric, nthreads=8)
    eb = oc.scores_all(B, q, metric, nthreads=8)
    assert eb.max() == ea[off].max() < ea[planted].min() and er.size == planted.size
    # one write of the run [first planted row, last planted row] carries every planted row and nothing else that differs
    lo, hi = int(planted.min()), int(planted.max())
    C = B.copy()
    C[lo:hi + 1] = A[lo:hi + 1]
    assert np.array_equal(C, A)


def test_model_takes_stale_maxima_only_where_it_is_given_them():
    A, q, k, metric, rows, info = ma.build("rows_i8", ma.DOT)
    m = ma.model(A, q, metric, "valu_i8")
    same = ma.model(A, q, metric, "valu_i8", maxima=(None, None, None))
    assert (same["rho_v"], same["e_abs"], same["max_norm"]) == (m["rho_v"], m["e_abs"], m["max_norm"])
    half = ma.model(A, q, metric, "valu_i8", maxima=(m["rho_v"] / 2, None, None))
    tau = float(np.sort(m["approx"])[-k])
    assert np.array_equal(half["approx"], m["approx"]) and half["rho_v"] == m["rho_v"] / 2
    assert tau - half["threshold"](tau) < 0.51 * (tau - m["threshold"](tau)), "the rows' rho_v is (almost) the whole margin"
    # the a-priori bound reads no measurement: stale maxima do not reach it
    A2, q2, _, _, _, _ = ma.build("rows_bf16", ma.COS)
    ap = ma.model(A2, q2, ma.COS, "mfma_f32", maxima=(0.0, 0.0, 0.0))
    assert ap["rho_v"] == 3.95e-3
