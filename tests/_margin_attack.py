"""Corpora and queries whose rounding errors are fully aligned against the right answer (docs/exactness.md, "The margins
under attack").  numpy and the oracle only; tests/test_margin_attack_cpu.py checks the constructions without a GPU,
tests/test_gpu_margin_attack.py searches them through every approximate sweep.

One pattern.  The coordinates split into a control part B (the first NB) and an error part G (the rest).
* G carries the error.  A planted row's G elements all sit next to one rounding midpoint of the stored format: the TARGET
  just on the side that lowers its approximate score, the DECOYS just on the other side.  The query (or, for the query
  attacks, the row) is parallel to that error on G, so |q . e_r| reaches |q||e_r| up to |q_G| / |q|.
* B carries no error (every value is exact in the stored format) and sets the exact order: the target's exact score is the
  best, the decoys follow strictly decreasing, a few distinct f32 scores apart.  B holds the pins (an element 127 that makes
  an 8-bit scale exactly 1) and a few LEVEL coordinates, coarse to fine, that `_fit` walks to put a score just below a goal.
* the bulk rows fill the shard; they score far below the planted rows and none has a larger rounding error.
The oracle then answers target, decoy 0, decoy 1 ...; in the mirror every decoy outranks the target by almost the whole 2E.

`model()` restates what each sweep stores (bf16 round-to-nearest-even; rint(x * 127 / max|x|), two query planes or one) and
the margin qprep_kernel / margin_key claim for it, in float64.  sharpness = (approximate score of the k-th decoy - approximate
score of the target) / (k-th decoy's approximate score - the collection threshold derived from it): 1 would be a target ON
the threshold, a margin worth half as much leaves every construction here outside it."""
import numpy as np

from oracle import oracle_c as oc

F = np.float32
U = 2.0 ** -24
NB = 10               # control coordinates: 0 the rows' pin, 1 the query's pin, 2.. the levels
P_ROW, P_QRY, L0 = 0, 1, 2
COS, L2, DOT = 0, 1, 2
K, N_DECOYS = 10, 12


# ---------------------------------------------------------------------------------------------- stored formats
def bf16(x):
    """float32 -> the bf16 value (as float32) the mirror and the matrix-core queries hold: round to nearest even."""
    b = np.ascontiguousarray(x, dtype=F).view(np.uint32)
    return ((b + np.uint32(0x7FFF) + ((b >> np.uint32(16)) & np.uint32(1))) & np.uint32(0xFFFF0000)).view(F)


def q8_codes(A):
    """Rows of float32 -> (scale f32 [n], codes f32 [n, d]): s = max|x| / 127, c = rint(x * (127 / max|x|)), f32 arithmetic."""
    A = np.atleast_2d(np.ascontiguousarray(A, dtype=F))
    mx = np.abs(A).max(axis=1)
    ok = mx > 0
    s = np.where(ok, mx / F(127.0), F(0)).astype(F)
    with np.errstate(divide="ignore"):
        inv = np.where(ok, F(127.0) / mx, F(0)).astype(F)
    t = (A * inv[:, None]).astype(F)
    return s, np.clip(np.rint(t), -127, 127).astype(F), t


def q8_rows(A):
    s, c, _ = q8_codes(A)
    return s.astype(np.float64)[:, None] * c.astype(np.float64)


def q8_query(q, planes):
    """The query the 8-bit sweeps multiply: s_q (h + l / 256), l = 0 with one plane."""
    s, h, t = q8_codes(q)
    l = np.clip(np.rint(((t - h).astype(F) * F(256.0)).astype(F)), -127, 127) if planes == 2 else np.zeros_like(h)
    return (s.astype(np.float64)[:, None] * (h.astype(np.float64) + l.astype(np.float64) / 256.0))[0]


# sweep -> (rows' format, query's format)
SWEEPS = {"valu_bf16": ("bf16", "f32"), "mfma_bf16": ("bf16", "bf16"), "mfma_f32": ("bf16_apriori", "bf16"),
          "valu_i8": ("i8", "i8x2"), "mfma_i8": ("i8", "i8x2"), "mfma_i8_one": ("i8", "i8x1")}


def stored(A, q, sweep):
    """(rows, query) as the sweep multiplies them, float64."""
    rf, qf = SWEEPS[sweep]
    At = q8_rows(A) if rf == "i8" else bf16(A).astype(np.float64)
    qt = {"f32": lambda: q.astype(np.float64), "bf16": lambda: bf16(q).astype(np.float64),
          "i8x2": lambda: q8_query(q, 2), "i8x1": lambda: q8_query(q, 1)}[qf]()
    return At, qt


def model(A, q, metric, sweep, maxima=None):
    """Approximate scores of every row and the claimed collection threshold as a function of the k-th approximate score.
    Returns dict(approx f64 [n], threshold callable, rho_v, e_abs, worst_rel_row, worst_abs_row).
    maxima = (rho_v, e_abs, max_norm): what the shard has MEASURED, where that is not what A's own rows give — the stale
    maxima of a shard whose writes did not raise them (written_attack); an entry of None keeps A's own."""
    A64, q64 = A.astype(np.float64), q.astype(np.float64)
    d = A.shape[1]
    At, qt = stored(A, q, sweep)
    vn = np.sqrt((A64 * A64).sum(axis=1))
    qn = np.sqrt((q64 * q64).sum())
    en = np.sqrt(((A64 - At) ** 2).sum(axis=1))
    rf, qf = SWEEPS[sweep]
    # the measured maxima with their slack (half_err_kernel / q8_err_kernel); a priori 3.95e-3 where nothing was measured
    with np.errstate(divide="ignore", invalid="ignore"):
        rel = np.where(vn > 0, en * 1.0005 / vn * 1.0005, 0.0)
    V = vn.max()
    if rf == "bf16_apriori":
        rho_v, e_abs = 3.95e-3, 3.95e-3 * V
    else:
        rho_v, e_abs = rel.max(), en.max() * 1.0005
        if maxima is not None:
            rho_v, e_abs, V = (own if m is None else m for m, own in zip(maxima, (rho_v, e_abs, V)))
    eq = np.sqrt(((q64 - qt) ** 2).sum()) * 1.0005
    rho_q = eq / qn if qf != "f32" else 0.0
    split = 2.0 * rho_v + (2.0 * rho_q * (1.0 + rho_v) * 1.0005 if qf != "f32" else 0.0)
    f32_term = 3.0 * (d + 10.0) * U
    pad = pad_sq = m_abs = m_rel = 0.0
    space = "score"          # where the margin is additive: the score, the distance, or the squared distance
    if metric == COS:
        approx = (At @ qt) / np.where(vn > 0, vn * qn, 1.0)
        m_abs = f32_term + split
    elif metric == DOT:
        approx = At @ qt
        m_abs, m_rel = (f32_term + split) * qn * V, 8.0 * U
    else:
        m_rel = 4.0 * (d + 8.0) * U
        if sweep == "valu_bf16":
            approx = 1.0 / (1.0 + np.sqrt(((q64[None, :] - At) ** 2).sum(axis=1)))
            pad, space = 2.0 * e_abs, "dist"
        elif sweep == "valu_i8":          # estimator A, |q~ - v~|
            approx = 1.0 / (1.0 + np.sqrt(((qt[None, :] - At) ** 2).sum(axis=1)))
            Vt, qq = V + e_abs, qn + eq
            pad, pad_sq, m_rel = 2.0 * 1.001 * (e_abs + eq), 2.0 * ((d / 64.0 + 16.0) * U) * (qq + Vt) ** 2, 16.0 * U
            space = "dist"
        elif sweep in ("mfma_bf16", "mfma_f32"):
            # estimator B: |q|^2 + |v|^2 - 2 q~.v~ with the exact magnitudes, a slightly negative result is a distance of 0;
            # the SQUARED distance is off by A = a_round + a_fp, the threshold distance d grows to sqrt(d^2 + 2 * 1.001 A)
            approx = 1.0 / (1.0 + np.sqrt(np.maximum(qn * qn + vn * vn - 2.0 * (At @ qt), 0.0)))
            a_round = 2.0 * qn * (e_abs + rho_q * (V + e_abs))
            a_fp = (d + 10.0) * U * (6.0 * qn * V + V * V + qn * qn) + 3.0 * U * (qn + V) ** 2
            pad_sq, m_rel, space = 2.0 * 1.001 * (a_round + a_fp), 16.0 * U, "dist2"
        else:
            raise ValueError("the 8-bit matrix-core Euclidean estimator is not modelled")

    def threshold(tau):
        if pad_sq > 0.0:
            dd = max(1.0 / tau - 1.0, 0.0) + pad
            tau = 1.0 / (1.0 + np.sqrt(dd * dd + pad_sq))
            return tau - abs(tau) * m_rel
        if pad > 0.0:
            tau = tau / (1.0 + pad * tau)
        return tau - m_abs - abs(tau) * m_rel

    return dict(approx=approx, threshold=threshold, space=space, rho_v=rho_v, e_abs=e_abs, rho_q=rho_q, max_norm=V,
                worst_rel_row=int(np.argmax(rel)), worst_abs_row=int(np.argmax(en)), worst_norm_row=int(np.argmax(vn)))


# ---------------------------------------------------------------------------------------------- the B part
def _fit(base, levels, q, metric, goal):
    """The planted row `base` with its level coordinates set so that the oracle's score is the largest one <= goal this
    greedy walk finds: level by level, coarse to fine, each level takes the option with the best score not above the goal
    while the finer levels still hold their option 0 (the lowest-scoring one).  levels: [(column, [values])]."""
    row = base.copy()
    for col, vals in levels:
        row[col] = vals[0]
    for col, vals in levels:
        cand = np.repeat(row[None, :], len(vals), axis=0)
        cand[:, col] = vals
        s = oc.scores_all(cand, q, metric)
        ok = np.nonzero(s <= goal)[0]
        if ok.size == 0:
            raise ValueError(f"level at column {col} cannot get below the goal {goal!r} (lowest {s.min()!r})")
        row[col] = vals[ok[np.argmax(s[ok])]]
    return row, oc.scores_all(row[None, :], q, metric)[0]


def _down(x, ulps):
    for _ in range(ulps):
        x = np.nextafter(F(x), F(-np.inf))
    return F(x)


def _plant(target_base, decoy_base, levels, q, metric, mid, n_decoys=N_DECOYS):
    """Target at the levels' middle, decoys below it one after the other, each 2 distinct f32 scores or a little more down."""
    t = target_base.copy()
    for (col, vals), m in zip(levels, mid):
        t[col] = vals[m]
    s_t = oc.scores_all(t[None, :], q, metric)[0]
    rows, scores, prev = [t], [s_t], s_t
    for _ in range(n_decoys):
        r, s = _fit(decoy_base, levels, q, metric, _down(prev, 2))
        rows.append(r)
        scores.append(s)
        prev = s
    return np.stack(rows).astype(F), np.array(scores, F)


def default_rows(n_rows, target_row, n_decoys=N_DECOYS):
    """Row ids of (target, decoys...): every planted row in a tile (64 rows) of its own, the decoys spread over the shard —
    the selection's bound is a k-th largest TILE maximum, so k decoys in one tile would not raise it."""
    tiles = n_rows // 64
    step = max((tiles - 2) // (n_decoys + 1), 1)
    out, t_tile = [target_row], target_row // 64
    tile = 1
    for j in range(n_decoys):
        tile += step
        if tile == t_tile:
            tile += 1
        out.append(tile * 64 + (37 * j + 5) % 64)
    assert len({r // 64 for r in out}) == len(out) and max(out) < n_rows
    return np.array(out, np.int64)


def _lin_levels(steps, count=256, first=0):
    return [(L0 + i, [F(n * s) for n in range(first, count)]) for i, s in enumerate(steps)]


# ---------------------------------------------------------------------------------------------- the constructions
# the margin's own space: scores, or for the Euclidean score 1 / (1 + d) the (negated) distance or squared distance
_SPACES = {"score": lambda s: s, "dist": lambda s: 1.0 - 1.0 / s, "dist2": lambda s: -(1.0 / s - 1.0) ** 2}


def _measure(m, pos, k):
    """(every row's approximate score, the k-th best decoy's, the collection threshold under it) of a model(), in the margin's
    own space.  pos: the planted rows, target first."""
    nat = _SPACES[m["space"]]
    a_k = np.sort(m["approx"][pos[1:]])[::-1][k - 1]          # the k-th best decoy in the mirror
    return nat(m["approx"]), nat(a_k), nat(m["threshold"](a_k))


def _finish(name, A, q, metric, rows, planted, exact, sweeps, floor, fmt, q_exact, note=""):
    """Plant, model and measure: the common tail of every construction."""
    A[rows] = planted
    k = K
    info = dict(name=name, metric=metric, target=int(rows[0]), decoys=rows[1:].copy(), exact_scores=exact, floor=floor,
                sweeps=sweeps, row_format=fmt, query_exact=q_exact, note=note, B=np.arange(NB), G=np.arange(NB, A.shape[1]))
    sharp = {}
    # (a large shard is modelled on its planted rows and a sample of the bulk)
    sub = np.arange(A.shape[0]) if A.shape[0] <= 65536 else np.unique(np.concatenate([rows, np.arange(4096)]))
    pos = np.searchsorted(sub, rows)
    bulk = np.ones(sub.size, bool)
    bulk[pos] = False
    for sw in sweeps:
        m = model(A[sub], q, metric, sw)
        a, a_k, thr = _measure(m, pos, k)
        sharp[sw] = dict(space=m["space"], sharpness=(a_k - a[pos[0]]) / (a_k - thr), E=(a_k - thr) / 2.0, a_k=a_k, a_target=a[pos[0]],
                         a_decoys=a[pos[1:]], best_bulk=a[bulk].max() if bulk.any() else -np.inf, rho_v=m["rho_v"], rho_q=m["rho_q"],
                         e_abs=m["e_abs"], max_norm=m["max_norm"], worst_rows=tuple(int(sub[m[w]]) for w in ("worst_rel_row", "worst_abs_row", "worst_norm_row")))
    info["by_sweep"] = sharp
    if floor is None:          # both_i8: what the better of its two parts, the rows', allows
        info["floor"] = 0.95 * min(v["rho_v"] / (v["rho_v"] + v["rho_q"] * (1.0 + v["rho_v"])) for v in sharp.values())
    info["sharpness"] = min(v["sharpness"] for v in sharp.values())
    return A, q.astype(F), k, metric, rows, info


def _bulk(n_rows, d, seed, bulk):
    return oc.synth(seed, 0, n_rows, d, nthreads=8) if bulk is None else bulk


def rows_bf16(metric, n_rows=8192, d=256, target_row=0, rows=None, bulk=None, bulk_scale=0.5, seed=0xA77AC0, n_decoys=N_DECOYS):
    """rho_v / D of the bf16 mirror (and, on the f32 matrix-core sweep, the a-priori 3.95e-3).  G: target 1 + 2^-8 - 2^-16
    (stored 1), decoys 1 + 2^-8 + 2^-16 (stored 1 + 2^-7); cosine / dot: q_G = 1; Euclidean: q_G = 1 + 2^-3, so that
    q - v is parallel to e_r on G and stays so in the mirror (the VALU sweep's |q - v~|), q itself is parallel to e_r (the
    matrix cores' |q|^2 + |v|^2 - 2 q.v~, off by 2 q . e_r on the SQUARED distance) and no decoy's estimate goes below zero.  The query is bf16-exact: the attack is on the rows alone."""
    A = _bulk(n_rows, d, seed, bulk)
    if bulk_scale != 1.0:
        A *= F(bulk_scale)
    rows = default_rows(n_rows, target_row, n_decoys) if rows is None else np.asarray(rows, np.int64)
    t, dc, q = np.zeros(d, F), np.zeros(d, F), np.zeros(d, F)
    t[NB:] = F(1.0 + 2.0 ** -8 - 2.0 ** -16)
    dc[NB:] = F(1.0 + 2.0 ** -8 + 2.0 ** -16)
    if metric == L2:
        # v_B = n * step approaches q_B = 256 * step from below: (256 - n)^2 step^2 of squared distance, ranges nested
        steps = [2.0 ** -8, 2.0 ** -11, 2.0 ** -14, 2.0 ** -17]
        q[NB:] = F(1.0 + 2.0 ** -3)
        for i, s in enumerate(steps):
            q[L0 + i] = F(256 * s)
        levels, mid = _lin_levels(steps, 257, 1), [239, 127, 127, 127]
    else:
        # q_B = -1: the score falls as v_B = n * step grows, for the dot product and (v_B >= 0) the cosine alike
        steps = [2.0 ** -8, 2.0 ** -13, 2.0 ** -18, 2.0 ** -23]
        q[NB:] = F(1.0)
        q[L0:L0 + 4] = F(-1.0)
        levels, mid = [(c, v[::-1]) for c, v in _lin_levels(steps)], [127, 127, 127, 127]
    planted, exact = _plant(t, dc, levels, q, metric, mid, rows.size - 1)
    sweeps = ["valu_bf16", "mfma_bf16", "mfma_f32"]
    return _finish("rows_bf16", A, q, metric, rows, planted, exact, sweeps, 0.95, "bf16", "bf16")


def _i8_levels(planes):
    # rows: integer codes 0..127 (option 0 = 127, the lowest score under a negative query element); the query's level
    # elements are exact in its own planes: integers with one plane, multiples of 1/256 with two
    qv = [-16.0, -1.0] + ([-2.0 ** -4, -2.0 ** -8] if planes == 2 else [])
    return qv, [(L0 + i, [F(n) for n in range(127, -1, -1)]) for i in range(len(qv))]


def _toggles(weights):
    # rows: +1 or -1 (the norm does not move), query: -w, so option 0 (+1) scores lowest; one toggle is worth 2 w of dot product
    return [-w for w in weights], [(L0 + i, [F(1.0), F(-1.0)]) for i in range(len(weights))]


# (two planes: no weight of 0.5 — h = rint(0.5) would be a tie, and l = 128 does not fit the second plane)
TOGGLES = {2: [4.0, 2.0, 1.0, 0.4375, 0.25, 0.125, 2.0 ** -4, 2.0 ** -5], 1: [32.0, 16.0, 8.0, 4.0, 2.0, 1.0]}


def rows_i8(metric, n_rows=8192, d=256, target_row=0, rows=None, planes=2, query_mid=False, seed=0xA77AC1, name="rows_i8"):
    """rho_v / E of the 8-bit mirror.  Rows: pin 127 (scale exactly 1), G at 32.5 -+ 2^-16 (stored 32 / 33).  Cosine / dot:
    q_G = 127 (its own pin: q~ = q in one plane already).  Euclidean (estimator A): q_G = 34 and its pin on the rows' pin,
    q - v parallel to e_r on G, in the mirror too; B: toggles q_B = n0 + f against v_B = n0 or n0 + 1 (two query planes).
    query_mid (both_i8): q_G at 126 + (0.5 - 2^-6) / 256 instead — between two codes of the SECOND plane, so the query's
    own rounding (rho_q) and the cross term rho_q rho_v are in the claimed margin as well."""
    A = _bulk(n_rows, d, seed, None)
    A *= F(16.0)
    rows = default_rows(n_rows, target_row) if rows is None else np.asarray(rows, np.int64)
    t, dc, q = np.zeros(d, F), np.zeros(d, F), np.zeros(d, F)
    t[NB:] = F(32.5 - 2.0 ** -16)
    dc[NB:] = F(32.5 + 2.0 ** -16)
    t[P_ROW] = dc[P_ROW] = F(127.0)
    if metric == L2:
        assert planes == 2 and not query_mid
        q[NB:] = F(34.0)
        q[P_ROW] = F(127.0)
        levels, mid = [], []
        for i, w in enumerate([64, 32, 16, 8, 4, 2, 1]):          # squared-distance weights (1 - 2 f) = 2 w / 256
            f = 0.5 - w / 256.0
            q[L0 + i] = F(40.0 + f)
            levels.append((L0 + i, [F(41.0), F(40.0)]))
            mid.append(1 if i == 0 else 0)
    else:
        qv, levels = _toggles(TOGGLES[planes])
        q[NB:] = F(127.0) if not query_mid else F(126.0 + (0.5 - 2.0 ** -6) / 256.0)
        q[P_QRY] = F(127.0)
        q[L0:L0 + len(qv)] = np.array(qv, F)
        mid = [1] + [0] * (len(qv) - 1)
    planted, exact = _plant(t, dc, levels, q, metric, mid)
    if planes == 1:
        sweeps = ["mfma_i8_one"]
    else:
        sweeps = ["valu_i8", "mfma_i8"] if metric == DOT and not query_mid else ["valu_i8"]
    return _finish(name, A, q, metric, rows, planted, exact, sweeps, None if query_mid else 0.95, "i8",
                   None if query_mid else ("i8x2" if planes == 2 else "i8x1"))


def both_i8(metric=COS, **kw):
    """rho_q (1 + rho_v) + rho_v together: rows_i8 with the query between two codes of its second plane.  With two planes
    rho_q (~2e-5) is far below rho_v (~0.015): the floor is the rows' 0.95 times rho_v's share rho_v / (rho_v + rho_q (1 + rho_v)) of the claimed sum,
    computed from the model (0.949)."""
    assert metric == COS
    return rows_i8(metric, query_mid=True, name="both_i8", seed=0xA77AC2, **kw)


def query_bf16(metric, n_rows=8192, d=256, target_row=0, rows=None, seed=0xA77AC3):
    """rho_q of the matrix-core sweeps' bf16 query.  Every row is bf16-exact (rho_v = 0 measured).  G in two halves: on the first
    q = 1 + 2^-8 - 2^-16 (stored 1: e_q < 0), on the second 1 + 2^-8 + 2^-16 (stored 1 + 2^-7: e_q > 0); the target is 1 on the
    first half and 0 on the second, the decoys the other way round — each sees |e_q| / sqrt 2 of the query's error."""
    assert metric in (COS, DOT)
    A = bf16(_bulk(n_rows, d, seed, None) * F(0.5)).copy()
    rows = default_rows(n_rows, target_row) if rows is None else np.asarray(rows, np.int64)
    h = NB + (d - NB) // 2
    t, dc, q = np.zeros(d, F), np.zeros(d, F), np.zeros(d, F)
    t[NB:h] = F(1.0)
    dc[h:] = F(1.0)
    q[NB:h] = F(1.0 + 2.0 ** -8 - 2.0 ** -16)
    q[h:] = F(1.0 + 2.0 ** -8 + 2.0 ** -16)
    q[L0:L0 + 4] = F(-1.0)
    steps = [2.0 ** -8, 2.0 ** -13, 2.0 ** -18, 2.0 ** -23]
    levels = [(c, v[::-1]) for c, v in _lin_levels(steps)]
    planted, exact = _plant(t, dc, levels, q, metric, [127] * 4)
    return _finish("query_bf16", A, q, metric, rows, planted, exact, ["mfma_bf16"], 0.65, "bf16", None)


def query_i8(metric, planes, n_rows=8192, d=256, target_row=0, rows=None, seed=0xA77AC4):
    """rho_q of the 8-bit query.  Every row is code-exact (integers, one element of magnitude 127: rho_v = 0 measured).
    One plane (cosine, the matrix-core batches of k <= 128): the two halves of query_bf16 with q at 32.5 -+ 2^-16 and rows of 100.
    Two planes: the query's rounding is 2^-9 of a code, rho_q <= 2^-9 sqrt(d) / 127 = 2.4e-4, and the f32 budget 3 (d + 10) u in the
    same margin is a tenth of 2 rho_q — the halves' 1 / sqrt 2 would end at 0.64.  So there q_G = (0.5 - 2^-6) / 256 on ALL of G
    (stored 0: e_q > 0), the target is +100 on G and the decoys are -100: both see all of |e_q|, and B makes up the exact difference."""
    assert (metric == COS and planes in (1, 2)) or (metric == DOT and planes == 2)
    A = np.clip(np.rint(_bulk(n_rows, d, seed, None) * F(20.0)), -126, 126).astype(F)
    A[:, P_QRY] = F(-127.0)                     # every bulk row's pin, against the query's: the bulk scores far below
    rows = default_rows(n_rows, target_row) if rows is None else np.asarray(rows, np.int64)
    t, dc, q = np.zeros(d, F), np.zeros(d, F), np.zeros(d, F)
    t[P_ROW] = dc[P_ROW] = F(127.0)
    q[P_QRY] = F(127.0)
    qv, levels = _toggles(TOGGLES[1]) if planes == 1 else _i8_levels(planes)
    mid = [1] + [0] * (len(qv) - 1) if planes == 1 else [63] * len(qv)
    q[L0:L0 + len(qv)] = np.array(qv, F)
    if planes == 1:
        h = NB + (d - NB) // 2
        t[NB:h] = F(100.0)
        dc[h:] = F(100.0)
        q[NB:h] = F(32.5 - 2.0 ** -16)
        q[h:] = F(32.5 + 2.0 ** -16)
        floor, sweeps = 0.65, ["mfma_i8_one"]
    else:
        t[NB:] = F(100.0)
        dc[NB:] = F(-100.0)
        q[NB:] = F((0.5 - 2.0 ** -6) / 256.0)
        floor, sweeps = 0.65, ["valu_i8", "mfma_i8"] if metric == DOT else ["valu_i8"]
    planted, exact = _plant(t, dc, levels, q, metric, mid)
    return _finish("query_i8", A, q, metric, rows, planted, exact, sweeps, floor, "i8", None)


# (name, metric, keyword arguments): every construction the tests run, once each
CASES = [("rows_bf16", COS, {}), ("rows_bf16", DOT, {}), ("rows_bf16", L2, {}),
         ("rows_i8", COS, {}), ("rows_i8", DOT, {}), ("rows_i8", L2, {}), ("rows_i8", COS, {"planes": 1}),
         ("query_bf16", COS, {}), ("query_bf16", DOT, {}),
         ("query_i8", COS, {"planes": 1}), ("query_i8", COS, {"planes": 2}), ("query_i8", DOT, {"planes": 2}),
         ("both_i8", COS, {})]
BUILDERS = {"rows_bf16": rows_bf16, "rows_i8": rows_i8, "query_bf16": query_bf16, "query_i8": query_i8, "both_i8": both_i8}
_memo = {}


def build(name, metric, **kw):
    """A construction, built once per argument set and shared (callers must not modify what they get)."""
    key = (name, metric, tuple(sorted((k, v if np.isscalar(v) else tuple(np.asarray(v).tolist())) for k, v in kw.items())))
    if key not in _memo:
        _memo[key] = BUILDERS[name](metric, **kw)
    return _memo[key]


# ---------------------------------------------------------------------------------------------- attacks that arrive by write
# (name, metric, keyword arguments, the model()'s sweep): every construction tests/test_gpu_write_paths.py writes into a shard
# whose mirror and error maxima already exist.  The f32 matrix-core sweep over a shard that holds a complete bf16 mirror
# takes that mirror's MEASURED maxima (search_enqueue) and rounds the rows as the mirror does: the mfma_bf16 model is its own.
WRITTEN_CASES = [("rows_bf16", COS, {}, "valu_bf16"), ("rows_bf16", DOT, {}, "valu_bf16"), ("rows_bf16", L2, {}, "valu_bf16"),
                 ("rows_bf16", COS, {}, "mfma_bf16"), ("rows_bf16", L2, {}, "mfma_bf16"),
                 ("rows_i8", COS, {}, "valu_i8"), ("rows_i8", DOT, {}, "valu_i8"), ("rows_i8", L2, {}, "valu_i8"),
                 ("rows_i8", DOT, {}, "mfma_i8"), ("rows_i8", COS, {"planes": 1}, "mfma_i8_one")]
_memo_written = {}


def written_attack(name, metric, **kw):
    """(B, A, q, k, planted, info): A is build(name, metric, **kw); B is A before its planted rows arrive — each planted slot
    holds a copy of the bulk row next to it (planted rows sit in tiles of their own, so a neighbour is bulk).  A shard that
    is uploaded as B, searched, and then has A's planted rows WRITTEN into it must end with A's mirror and A's error maxima.
    info (a copy of A's) gains, per modelled sweep,
      stale_sharpness      (k-th decoy - target) / the margin claimed from B's rho_v, e_abs and max_norm: above 1 the target
                           is outside a margin whose maxima no write has raised;
      stale_err_sharpness  the same with B's rho_v and e_abs but A's max_norm (the magnitudes are kept by another word);
      stale_maxima         B's (rho_v, e_abs, max_norm).
    Built once per argument set and shared: callers must not modify what they get."""
    key = (name, metric, tuple(sorted(kw.items())))
    if key in _memo_written:
        return _memo_written[key]
    A, q, k, _, planted, info = build(name, metric, **kw)
    assert A.shape[0] <= 65536
    B = A.copy()
    own = set(planted.tolist())
    for r in planted:
        nb = int(r) + 1 if int(r) + 1 < A.shape[0] else int(r) - 1
        assert nb not in own and nb // 64 == int(r) // 64
        B[r] = A[nb]
    info = dict(info, stale_sharpness={}, stale_err_sharpness={}, stale_maxima={})
    for sw in info["sweeps"]:
        if SWEEPS[sw][0] == "bf16_apriori":          # nothing measured, nothing to go stale
            continue
        mb = model(B, q, metric, sw)
        stale = (mb["rho_v"], mb["e_abs"], mb["max_norm"])
        info["stale_maxima"][sw] = stale
        for field, maxima in (("stale_sharpness", stale), ("stale_err_sharpness", (stale[0], stale[1], None))):
            a, a_k, thr = _measure(model(A, q, metric, sw, maxima=maxima), planted, k)
            info[field][sw] = (a_k - a[planted[0]]) / (a_k - thr)
    _memo_written[key] = (B, A, q, k, planted, info)
    return _memo_written[key]
