"""Every approximate sweep's candidate margin under worst-case rounding errors (docs/exactness.md, "The margins under attack").

The corpora of tests/_margin_attack.py put a target row just below a rounding midpoint and at least k decoys just above it,
with the query along the error: in the mirror every decoy outranks the target by almost the whole claimed 2E, while the
oracle's answer starts with the target.  A margin that applied an error once instead of twice, dropped rho_q or rho_v, or was
forgotten in a score-store bound loses the target and fails here; the synthetic and N(0,1) corpora of the other tests stay one
to two orders of magnitude inside every margin and cannot tell.

Every case checks rows, counts and score bits against the oracle, that the sweep under attack is the one that ran, that no query
fell back to the exact scan, and that no more rows were re-scored than were planted: the candidate path answered, and the bulk
stayed outside the margin."""
import numpy as np
import pytest

from oracle import oracle_c as oc
from tests import _margin_attack as ma

pytestmark = pytest.mark.gpu
F = np.float32
COS, L2, DOT = ma.COS, ma.L2, ma.DOT
N = 8192                 # rows of the default constructions (x 256 elements): above the 8-bit mirror's smallest shard (4096 rows);
                         # the stride is a multiple of 128 (the 8-bit VALU sweep) and of 256 (the 8-bit matrix-core sweep)


def _batch(q, layout, seed=5):
    """The attacking query alone ("1"), or among ordinary ones — its own neighbourhood, 3 % of noise per element — at the
    first ("2a", "8a") or the last position ("2b", "8b") of a call."""
    if layout == "1":
        return q[None, :].copy(), 0
    nq, at = int(layout[0]), (0 if layout[1] == "a" else int(layout[0]) - 1)
    rng = np.random.default_rng(seed)
    Q = (q[None, :] * (1.0 + 0.03 * rng.standard_normal((nq, q.size)))).astype(F)
    Q[at] = q
    return Q, at


def _check(idx, A, Q, k, metric, sweep, planted, mask=None, crowd=False):
    rows, scores, counts, st = idx.search(Q, k, metric, mask=mask, with_stats=True)
    print(f"sweep {st.sweep}, launches {st.sweep_launches}, candidates {st.candidates_rescored}, fallback {st.fallback_queries}")
    assert st.sweep == sweep, (st.sweep, sweep)
    for i in range(Q.shape[0]):
        er, es = oc.search(A, Q[i], k, metric, mask=mask, nthreads=8, partial=True, native=True)
        assert counts[i] == er.size, (i, int(counts[i]), er.size)
        assert np.array_equal(rows[i, :er.size], er), (i, rows[i, :er.size], er)
        assert np.array_equal(scores[i, :er.size].view(np.uint32), es.view(np.uint32)), (i, scores[i, :er.size], es)
    assert st.fallback_queries == 0
    if not crowd:
        assert st.candidates_rescored <= planted, (st.candidates_rescored, planted)
    return st


def _kw_id(kw):
    return "".join(f"-{k}{v}" for k, v in sorted(kw.items()))


def _cases():
    out = []

    def add(name, metric, kw, mode, sweep, layouts, masked=False):
        for lay in layouts:
            out.append(pytest.param(name, metric, kw, mode, sweep, lay, masked,
                                    id=f"{sweep}-{name}-{'cos l2 dot'.split()[metric]}{_kw_id(kw)}-{lay}{'-bitmap' if masked else ''}"))

    for m in (COS, DOT, L2):
        add("rows_bf16", m, {}, 2, "valu_bf16", ["1"])
        add("rows_i8", m, {}, 1, "valu_i8", ["1", "2a", "2b"])
    for m in (COS, DOT):
        add("query_i8", m, {"planes": 2}, 1, "valu_i8", ["1", "2b"])
        add("rows_bf16", m, {}, 2, "mfma_bf16", ["8a", "8b"])
        add("query_bf16", m, {}, 2, "mfma_bf16", ["8a", "8b"])
        add("rows_bf16", m, {}, 0, "mfma_f32", ["8a", "8b"])          # no mirror: the a-priori 3.95e-3
    # the matrix cores' Euclidean estimator |q|^2 + |v|^2 - 2 q.v~: its margin is on the squared distance
    add("rows_bf16", L2, {}, 2, "mfma_bf16", ["8a", "8b"])
    add("rows_bf16", L2, {}, 0, "mfma_f32", ["8a", "8b"])
    add("both_i8", COS, {}, 1, "valu_i8", ["1", "2a"])
    # batches on the 8-bit mirror: cosine with k <= 128 multiplies ONE query plane, the dot product both
    add("rows_i8", COS, {"planes": 1}, 1, "mfma_i8", ["8a", "8b"])
    add("query_i8", COS, {"planes": 1}, 1, "mfma_i8", ["8a", "8b"])
    add("rows_i8", DOT, {}, 1, "mfma_i8", ["8a"])
    add("query_i8", DOT, {"planes": 2}, 1, "mfma_i8", ["8b"])
    # the target at row 63, row 64 and the last row (row 0 above); under a bitmap: the masked sweep and the survivor walk
    for pos in (63, 64, N - 1):
        add("rows_bf16", COS, {"target_row": pos}, 2, "valu_bf16", ["1"])
        add("rows_i8", COS, {"target_row": pos}, 1, "valu_i8", ["1"])
    add("rows_bf16", COS, {}, 2, "valu_bf16", ["1"], masked=True)
    add("rows_i8", COS, {}, 1, "valu_i8", ["1"], masked=True)
    return out


@pytest.mark.parametrize("name,metric,kw,mode,sweep,layout,masked", _cases())
def test_margin_holds_under_attack(name, metric, kw, mode, sweep, layout, masked):
    from neumann_amd import GpuFlatIndex
    A, q, k, _, planted, info = ma.build(name, metric, **kw)
    model = "mfma_i8_one" if (sweep == "mfma_i8" and metric == COS) else sweep
    assert model in info["by_sweep"], "the construction was not built for this sweep"
    v = info["by_sweep"][model]
    print(f"{name}: sharpness {v['sharpness']:.4f} of the claimed margin, E {v['E']:.4g}, rho_v {v['rho_v']:.4g}, rho_q {v['rho_q']:.4g}")
    assert info["floor"] <= v["sharpness"] < 1.0
    Q, _ = _batch(q, layout)
    mask = None
    if masked:
        keep = np.random.default_rng(17).random(A.shape[0]) < 0.2
        keep[planted] = True
        mask = oc.mask_from_bool(keep)
    with GpuFlatIndex(A.shape[1], A.shape[0], single_launch=False) as idx:
        idx.set_mirror(mode)          # before the rows arrive: mode 0 builds no mirror, so nothing is measured
        idx.upload(A)
        _check(idx, A, Q, k, metric, sweep, planted.size, mask=mask)


# ---------------------------------------------------------------------------------------------- the store bounds
BIG_N, BIG_D = 32768 * 64, 128          # 32 768 tiles: the smallest shard whose batches gate their score stores by a bound


@pytest.fixture(scope="module")
def big():
    """2M x 128, synthetic bulk, a rows_bf16 cosine attack planted with set_row, for the LAST query of a batch of 8.
    The sweep's 1024 workgroups own 32 tiles each and go round the 8 XCDs (workgroup b on XCD b % 8).  The running bound of query 7
    is refreshed by the workgroups b = 7 (mod 64), at their tile 7, from the workgroups' running maxima — plain stores, which a
    reader on another XCD need not see yet.  So the decoys open the FIRST tile of the workgroups 15, 23, ... 103: the same XCD
    as those refreshers, in the first round of workgroups, published seven tiles before workgroup 7 asks.  Their tiles are
    multiples of 32, tiles of the sampling pass as well.  The target is the last row of the shard: the last tile of workgroup 1023,
    on that XCD again, in the last round, in a tile no sample sees."""
    from neumann_amd import GpuFlatIndex
    seed = 0xB16
    rows = [BIG_N - 1] + [32 * (7 + 8 * (j + 1)) * 64 + (37 * j + 5) % 64 for j in range(ma.N_DECOYS)]
    bulk = oc.synth(seed, 0, BIG_N, BIG_D, nthreads=8)
    A, q, k, metric, planted, info = ma.rows_bf16(COS, n_rows=BIG_N, d=BIG_D, rows=rows, bulk=bulk, bulk_scale=1.0)
    v = info["by_sweep"]["mfma_bf16"]
    assert info["floor"] <= v["sharpness"] < 1.0 and set(v["worst_rows"][:1]) <= set(planted.tolist())
    with GpuFlatIndex(BIG_D, BIG_N, single_launch=False) as idx:
        idx.set_mirror(2)
        idx.fill_synthetic(seed, BIG_N)
        for r in planted:
            idx.set_row(int(r), A[r])
        yield idx, A, q, k, planted


@pytest.mark.parametrize("layout", ["8a", "8b"])
def test_running_bound_leaves_the_margin_its_room(big, layout):
    """The one-launch batch (ScanParams::run_*: unmasked, k <= 256, >= 32 768 tiles).  The planting of `big` is what makes the
    bound matter: with the decoys on other XCDs than the refreshing workgroups (first tiles of workgroups 1 .. 12) the bound
    never rose to them before the sweep ended, and a build whose running bound left out margin_key passed; planted as now, that
    build loses the target at both positions of the attacking query (the other queries are its 3 % neighbours, attacks of
    their own)."""
    idx, A, q, k, planted = big
    Q, _ = _batch(q, layout)
    st = _check(idx, A, Q, k, COS, "mfma_bf16", planted.size)
    assert st.sweep_launches == 1, "the running bound replaces the sampling pass"


def test_sampled_bound_leaves_the_margin_its_room(big):
    """The sampling pass + sample_bound_kernel: what a batch under a bitmap takes on the same shard."""
    idx, A, q, k, planted = big
    keep = np.random.default_rng(23).random(BIG_N) < 0.2
    keep[planted] = True
    Q, _ = _batch(q, "8b")
    st = _check(idx, A, Q, k, COS, "mfma_bf16", planted.size, mask=oc.mask_from_bool(keep))
    assert st.sweep_launches >= 3, "sampling pass, bound, main sweep"


def test_crowd_list_takes_the_rows_inside_the_margin():
    """2^18 x 128, 200 decoys, candidate lists of 64: the rows inside the margin overflow the list and go through
    crowd_count / crowd_fill — all of them, the target included — instead of the exact fallback."""
    from neumann_amd import GpuFlatIndex
    n, d, cap = 1 << 18, 128, 64
    A, q, k, metric, planted, info = ma.build("rows_bf16", COS, n_rows=n, d=d, n_decoys=200, bulk_scale=1.0, seed=4711)
    assert info["floor"] <= info["by_sweep"]["valu_bf16"]["sharpness"] < 1.0 and planted.size == 201
    with GpuFlatIndex(d, n, single_launch=False, cand_cap=cap) as idx:
        idx.set_mirror(2)
        idx.upload(A)
        st = _check(idx, A, q[None, :], k, COS, "valu_bf16", planted.size, crowd=True)
        assert st.candidates_rescored == planted.size > cap, "all 201 rows inside the margin went through the crowd list, and only they"
