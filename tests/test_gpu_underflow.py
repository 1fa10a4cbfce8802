"""Every approximate sweep at the f32 underflow edge, against the oracle (docs/exactness.md §4, "The underflow guard").

The candidate margins that make the approximate sweeps exact were derived for f32 arithmetic without underflow: the
measured quantization errors are sums of e*e, the dot-product margin scales with the largest stored magnitude, and the f32
term 3 (d + 10) u assumes fl(a b) = a b (1 + delta).  On shards whose squares or products underflow — whole shards scaled
to 1e-19 ... 1e-44, the straddle row 767 x 2.5e-23 + 4e-23 whose stored magnitude is 18.5x below the true one, tiny rows
planted among normal ones — those margins can come out too small, and the guard in qprep_kernel must send the query to the
exact path instead.  These tests force every sweep kind (the recipe of test_gpu_sweep_kind.py) over such shards with
normal, tiny and zero queries and check the answers: rows identical, scores as u32 bits (the sign of an all-zero sum
aside), counts and the U64_MAX / -inf padding.  On the normal control corpus they also check that normal queries stay on
the requested sweep with no fallback, so a guard that sends normal data to the exact path fails here too."""
import numpy as np
import pytest

from oracle import oracle_c as oc
from tests import _corpora as shared

pytestmark = pytest.mark.gpu
F = np.float32
U64_MAX = np.uint64(0xFFFFFFFFFFFFFFFF)
N, D = 270_000, 256          # >= 4096 tiles (ring), stride a multiple of 256 (8-bit matrix-core sweep)
STRADDLE = shared.STRADDLE

# (mirror mode, queries per call, bitmap?) -> the sweep that must serve it on the control corpus
SWEEPS = [(0, 1, False, "ring_f32"), (0, 1, True, "valu_f32"), (0, 2, False, "valu_f32"), (2, 1, False, "valu_bf16"),
          (1, 1, False, "valu_i8"), (0, 8, False, "mfma_f32"), (2, 8, False, "mfma_bf16"), (1, 8, False, "mfma_i8"),
          (1, 8, True, "mfma_i8")]


def _ranked(scores, part, k):
    """The reference's order (score descending, NaN last, then row) over the rows `part`, top k."""
    s = scores[part].astype(np.float64)
    order = np.lexsort((part, np.where(np.isnan(s), np.inf, -s)))[:k]
    return part[order].astype(np.uint64), scores[part][order].astype(F)


class Oracle:
    """Each oracle answer once per (query, metric, mask), at the largest k asked of it; smaller k are its prefixes."""

    def __init__(self, A):
        self.A = A
        self.memo = {}

    def answer(self, q, k, metric, mask=None, mkey=None):
        key = (q.tobytes(), metric, mkey)
        kk = max(k, 100)
        hit = self.memo.get(key)
        if hit is None or hit[0] < kk:
            if metric != 1 and float(oc.magnitude(q)) == 0.0:
                # |q| == 0 — a zero query, or one whose squares all underflow: the facade answers `Ok([])` (lib.rs:2066),
                # the C ABI scores every row (cosine 0.0, dot products as they come), as in test_gpu_fuzz.py
                with np.errstate(all="ignore"):
                    s = oc.scores_all(self.A, q, metric, nthreads=8, native=True)
                part = np.arange(self.A.shape[0]) if mask is None else np.nonzero(
                    np.unpackbits(mask.view(np.uint8), bitorder="little")[:self.A.shape[0]])[0]
                er, es = _ranked(s, part, kk)
            else:
                er, es = oc.search(self.A, q, kk, metric, mask=mask, nthreads=8, partial=True, native=True)
            hit = (kk, er, es)
            self.memo[key] = hit
        return hit[1][:k], hit[2][:k]


def check(idx, orc, Q, k, metric, mask=None, mkey=None, what=""):
    Q = np.atleast_2d(Q)
    rows, scores, counts, st = idx.search(Q, k, metric, mask=mask, with_stats=True)
    for qi in range(Q.shape[0]):
        er, es = orc.answer(Q[qi], k, metric, mask, mkey)
        c = er.size
        ctx = (what, f"served by {st.sweep}", f"fallback {st.fallback_queries}", f"metric {metric}", f"k {k}", f"query {qi}")
        assert counts[qi] == c, ctx + (int(counts[qi]), c)
        assert np.array_equal(rows[qi, :c], er), ctx + (rows[qi, :6], er[:6])
        got = scores[qi, :c]
        # scores as bits; the sign of an all-zero sum is the one freedom the reference's order leaves (oracle/nmn_oracle.c)
        same = (got.view(np.uint32) == es.view(np.uint32)) | ((got == 0) & (es == 0))
        assert np.all(same), ctx + (got[~same][:4], es[~same][:4])
        assert np.all(rows[qi, c:] == U64_MAX) and np.all(np.isneginf(scores[qi, c:])), ctx
    return st


def _queries(rng, A, tiny_row):
    """8 queries: normal ones, tiny ones (1e-21, 1e-30 scaled), a copy of row `tiny_row` (a tiny row on the edge corpora)
    and the zero query."""
    z = np.zeros(D, F)
    g = lambda s: (rng.standard_normal(D) * s).astype(F)  # noqa: E731
    return np.stack([g(1.0), g(1e-21), A[tiny_row].copy(), z, g(1e-30), g(1.0), A[7].copy(), g(1e-21)]).astype(F)


def _straddle_rows(rng, m, d=D):
    return shared.straddle_rows(rng, m, d)


def _control():
    base = oc.synth(0x0DF0, 0, N, D, nthreads=8)
    return (base / np.float32(np.abs(base[:1000]).std())).astype(F)  # ~N(0,1)-sized


def _corpora():
    """(name, rows, row the copy query takes) for the control corpus and each edge corpus."""
    rng = np.random.default_rng(0x0DF1)
    base = _control()
    yield "control", base, 0
    for s in (1e-12, 1e-19, 1e-21, 1e-22, 1e-30, 1e-44):
        yield f"scale {s:g}", (base * F(s)).astype(F), 11
    # straddle: every row tiny; 400 near-ties of one row (one element swapped between 2.5e-23 and 4e-23) around the cut
    A, tie = shared.straddle_corpus(rng, N, D)
    yield "straddle", A, int(tie[1])
    # mixed: normal rows plus planted tiny rows whose inflated cosines (> 1) belong in the normal queries' top k
    A = base.copy()
    Q0 = _queries(np.random.default_rng(0x0DF2), A, 0)
    plant = rng.choice(np.arange(8, N), 3 * 60, replace=False)
    for j, qi in enumerate((0, 5, 6)):
        rows = plant[60 * j: 60 * (j + 1)]
        A[rows] = shared.tiny_rows_along(rng, Q0[qi], rows.size)
    yield "mixed", A, int(plant[0])
    # the upper end: +-1e6 everywhere (the reference fuzz target's bound), a few rows near 2e19 (|v|^2 overflows: |v| = inf)
    A = rng.uniform(-1e6, 1e6, (N, D)).astype(F)
    big = rng.choice(np.arange(8, N), 5, replace=False)
    A[big] = (2e19 * (1 + 0.1 * rng.random((5, D)))).astype(F) * rng.choice(np.array([-1, 1], F), (5, D))
    yield "upper", A, int(rng.integers(8, N))


def test_every_sweep_at_the_f32_range_edges():
    """Every corpus of _corpora() through every forced sweep, 1 / 2 / 8 queries per call (8: the matrix-core sweeps; cosine
    with k <= 128 on the 8-bit mirror is the one-plane query form), three metrics, k = 1 and 100, plus Euclidean top-1000
    under a bitmap (BASELINE config 5's shape).  Every failing case is collected, so one run lists them all."""
    from neumann_amd import GpuFlatIndex
    keep = np.random.default_rng(3).random(N) < 0.4
    mask = oc.mask_from_bool(keep)
    Qn = np.random.default_rng(0x0DF6).standard_normal((8, D)).astype(F)
    failures = []
    for name, A, copy_row in _corpora():
        Q = _queries(np.random.default_rng(0x0DF2), A, copy_row)
        orc = Oracle(A)
        with GpuFlatIndex(D, N, single_launch=False) as idx:
            idx.upload(A)
            for mode, nq, masked, kind in SWEEPS:
                idx.set_mirror(mode)
                m, mk = (mask, "0.4") if masked else (None, None)
                for metric in (0, 1, 2):
                    for k in (1, 100):
                        for qq in [Q[i:i + nq] for i in range(0, 8, nq)]:
                            try:
                                check(idx, orc, qq, k, metric, mask=m, mkey=mk, what=(name, kind))
                            except AssertionError as e:
                                failures.append(str(e).splitlines()[0][:200])
                        if name == "control":
                            # normal data must stay on the requested sweep, with no query sent to the exact path
                            st = check(idx, orc, Qn[:nq], k, metric, mask=m, mkey=mk, what=(name, kind, "normal"))
                            assert st.sweep == kind and st.fallback_queries == 0, (kind, metric, k, st.sweep, st.fallback_queries)
            idx.set_mirror(1)
            for qq in (Q[:1], Q):
                try:
                    check(idx, orc, qq, 1000, 1, mask=mask, mkey="0.4", what=(name, "k1000"))
                except AssertionError as e:
                    failures.append(str(e).splitlines()[0][:200])
    assert not failures, f"{len(failures)} cases differ from the oracle:\n" + "\n".join(failures)


def test_overwrites_and_appends_of_tiny_rows_after_the_mirrors_exist():
    """A normal shard whose 8-bit and bf16 mirrors exist: one row overwritten with a straddle row (set_row), tiny rows
    appended; every mirror mode searched again.  The write path must record the new rows' smallest element (nmn_api.hip
    rows_written), or the guard misses them: the shard's mirrors and largest magnitude still come from the normal rows."""
    from neumann_amd import GpuFlatIndex
    rng = np.random.default_rng(0x0DF3)
    n0, extra = N - 2000, 2000
    A = rng.standard_normal((N, D)).astype(F)
    Q = rng.standard_normal((8, D)).astype(F)
    with GpuFlatIndex(D, N, single_launch=False) as idx:
        idx.upload(A[:n0])
        for mode in (1, 2, 0):
            idx.set_mirror(mode)
            idx.search(Q[:1], 10, 0)
            idx.search(Q, 10, 0)
        s = _straddle_rows(rng, 1)[0]
        A[4321] = (np.abs(s) * np.sign(Q[0])).astype(F)            # inflated cosine > 1 for query 0: it belongs first
        idx.set_row(4321, A[4321])
        A[n0:] = (rng.standard_normal((extra, D)) * 1e-21).astype(F)
        A[n0 + 5] = (np.abs(_straddle_rows(rng, 1)[0]) * np.sign(Q[1])).astype(F)
        idx.upload(A[n0:])
        orc = Oracle(A)
        for mode in (1, 2, 0):
            idx.set_mirror(mode)
            for qq in (Q[:1], Q[:2], Q):
                for metric in (0, 1, 2):
                    check(idx, orc, qq, 100, metric, what=("overwrite+append", mode))


def test_a_tiny_shard_after_save_and_load(tmp_path):
    """A 1e-21 shard with straddle rows, saved and loaded: the load's upload records the smallest element again."""
    from neumann_amd import GpuFlatIndex
    rng = np.random.default_rng(0x0DF4)
    n = 270_000
    A = (rng.standard_normal((n, D)) * 1e-21).astype(F)
    A[100:140] = _straddle_rows(rng, 40)
    A[7] = 0.0
    Q = np.stack([rng.standard_normal(D).astype(F), (rng.standard_normal(D) * 1e-21).astype(F), A[120]]).astype(F)
    path = tmp_path / "tiny.nmnidx"
    with GpuFlatIndex(D, n) as idx:
        idx.upload(A)
        idx.save(path)
    orc = Oracle(A)
    with GpuFlatIndex.load(path, capacity_rows=n) as idx:
        for mode in (1, 2, 0):
            idx.set_mirror(mode)
            for qq in (Q[:1], Q[1:2], Q[2:3], Q):
                for metric in (0, 1, 2):
                    check(idx, orc, qq, 50, metric, what=("loaded", mode))


def test_engine_with_tiny_embeddings_matches_oracle():
    """VectorEngine: the reference stores |x| <= 1e-6 as sparse zeros for its density test (lib.rs:1876-1885) but keeps
    the values, so tiny embeddings are searched at their own scale."""
    from neumann_amd import engine as E
    rng = np.random.default_rng(0x0DF5)
    n, d, k = 6000, 96, 40
    A = (rng.standard_normal((n, d)) * 1e-21).astype(F)
    A[:300] = _straddle_rows(rng, 300, d)
    A[300:600] = (rng.standard_normal((300, d)) * 1e-30).astype(F)
    A[600:900] = rng.standard_normal((300, d)).astype(F)
    engine = E.VectorEngine()
    engine.batch_store_embeddings([f"k{i}" for i in range(n)], A)
    for q in (rng.standard_normal(d).astype(F), (rng.standard_normal(d) * 1e-21).astype(F), A[17].copy()):
        for metric in E.DistanceMetric:
            res = engine.search_similar_with_metric(q, k, metric)
            er, es = oc.search(A, q, k, int(metric))
            assert [r.key for r in res] == [f"k{i}" for i in er], metric
            assert np.array_equal(np.array([r.score for r in res], F).view(np.uint32), es.view(np.uint32)), metric


@pytest.mark.parametrize("scale", [1e-21, 1e-30])
def test_ivf_flat_on_a_tiny_corpus(scale):
    """IVF-Flat at the size test_gpu_ivf.py uses: the k-means and the centroid ranking both work on squared distances."""
    from neumann_amd.ivf import GpuIvfFlat
    from oracle import ivf_oracle as io
    rng = np.random.default_rng(5000 + int(-np.log10(scale)))
    n, d, c = 5000, 96, 50
    V = (rng.standard_normal((n, d)) * scale).astype(F)
    V[11] = V[5]
    orc = io.IVFFlat(c, nprobe=7, kmeans=io.KMeansConfig(max_iterations=5, convergence_threshold=1e-4, seed=7, init_method="kmeans++"))
    orc.train(V[:600])
    with GpuIvfFlat(orc.centroids, capacity_rows=n + 64, nprobe=orc.nprobe) as gpu:
        got = gpu.add(V)
        for v in V:
            orc.add(v)
        assert got.tolist() == orc.assign
        Q = (rng.standard_normal((3, d)) * scale).astype(F)
        for q in list(Q) + [V[5]]:
            for k in (1, 10, 200):
                ids, dist, counts = gpu.search(q, k)
                eids, ed = orc.search(q, k)
                assert counts[0] == len(eids)
                assert ids[0, :len(eids)].tolist() == eids
                assert np.array_equal(dist[0, :len(eids)], ed)  # (as test_gpu_ivf.py: a zero distance may come back as -0.0)
                assert np.all(ids[0, len(eids):] == U64_MAX) and np.all(np.isposinf(dist[0, len(eids):]))
