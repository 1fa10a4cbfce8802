"""Call kinds and call orders of tests/test_gpu_call_history.py (numpy + the oracle, no GPU).

A search on a shard is a chain of dependent launches whose bookkeeping words (row totals of the crowd kernels, the grid barrier of
the device-wide select, the meeting places of the split selection, ticket counters, the ring sweep's wave maxima, the histogram
the large-k path borrows) are never cleared in front of a call: every kernel leaves them the way the next call needs them
(docs/exactness.md, "Calls do not see each other").  So an answer could depend on the call BEFORE it, and only for some pairs of
paths.  This module provides

* `circuit(K)`: a closed walk over K call kinds in which every ordered pair of kinds, a kind followed by itself included, occurs
  exactly once as two consecutive calls;
* three palettes of call kinds, each on one shard: L (270 000 x 256: the eight sweeps, survivor walk, crowd list, bf16 overflow,
  k = 4096, both large-k forms, predicates, the certificate), T (300 000 x 32 identical rows: every query ends in the exact fallback
  with the device-wide select) and S (6 000 x 16 with 4 500 duplicates on a default index: the single launch beside the chain);
* per kind the oracle's answer, computed once, and the path fingerprint the call must report (`fingerprint`).
"""
import functools
from dataclasses import dataclass, field

import numpy as np

from neumann_amd import _capi
from oracle import oracle_c as oc
from tests import _corpora

F = np.float32
NO_ROW = np.uint64(0xFFFFFFFFFFFFFFFF)
COS, L2, DOT = 0, 1, 2
SWEEP_NAMES = {_capi.SWEEP_NONE: "none", _capi.SWEEP_RING_F32: "ring_f32", _capi.SWEEP_VALU_F32: "valu_f32",
               _capi.SWEEP_VALU_BF16: "valu_bf16", _capi.SWEEP_VALU_I8: "valu_i8", _capi.SWEEP_MFMA_F32: "mfma_f32",
               _capi.SWEEP_MFMA_BF16: "mfma_bf16", _capi.SWEEP_MFMA_I8: "mfma_i8", _capi.SWEEP_EXACT: "exact"}


def circuit(K):
    """Eulerian circuit of the complete digraph on 0..K-1 with loops (Hierholzer, every node's out-edges taken in ascending
    order): K*K + 1 entries, first == last, every ordered pair (a, b) exactly once as consecutive entries."""
    nxt = [0] * K          # the next unused out-edge of each node
    stack, out = [0], []
    while stack:
        v = stack[-1]
        if nxt[v] < K:
            nxt[v] += 1
            stack.append(nxt[v] - 1)
        else:
            out.append(stack.pop())
    out.reverse()
    return out


def fingerprint(stats, dim, crowd_min=0, fits=False):
    """What nmn_search_stats says about the path a call took, as a tuple:

    * the sweep kind by name;
    * the bytes per corpus element of the call's first sweep;
    * the number of queries answered by the exact fallback;
    * with `crowd_min`: whether at least that many rows were re-scored, which only the crowd list can do (the candidate list
      holds 4096);
    * with `fits`: whether what was re-scored fits the candidate list.  With a fallback count of 0 that rules out the crowd
      list and the exact fallback.  It does NOT show that a first selection overflowed:
      test_gpu_call_history.py::test_the_retry_kind_is_counted_as_retried_and_the_near_kind_is_not observes that.

    candidates_rescored itself is left out.  nmn_select.hip:951-954 stores the threshold distance of the last Euclidean
    selection on the 8-bit mirror in the shard's q8_l2_hint, and qprep_kernel of the NEXT such call picks its estimator from it
    (docs/exactness.md: "the choice moves the candidate count, never the answer")."""
    rescored = int(stats.candidates_rescored)
    eb = int(stats.bytes_scanned) // max(int(stats.rows_scanned) * dim, 1)
    fp = (SWEEP_NAMES.get(int(stats.sweep_kind), str(int(stats.sweep_kind))), eb, int(stats.fallback_queries))
    if crowd_min:
        fp += (rescored >= crowd_min,)
    if fits:
        fp += (rescored <= _capi.MAX_TOP_K,)
    return fp


@dataclass
class Kind:
    name: str
    op: str                 # "search" | "pred" | "count"
    mirror: int             # nmn_index_set_mirror before the call
    Q: np.ndarray           # [nq, d]
    k: int
    metric: int
    keep: np.ndarray = None     # bool [n]: the bitmap (op "search") or what the predicate selects (op "pred")
    pred: tuple = None          # ("lt" | "eq", value) on the palette's integer column
    fp: tuple = None            # expected fingerprint; None: the call reports no statistics (count_exact)
    crowd_min: int = 0          # fingerprint: at least this many rows re-scored (the crowd list)
    fits: bool = False          # fingerprint: what was re-scored fits the candidate list
    flags: bool = False         # a first selection of the call overflows: on a shard of >= 2^18 rows the host API's short chain
                                # comes back flagged, the call is run again with the whole chain and the next 256 host calls
                                # enqueue the whole chain at once (nmn_api.hip: short_off_until)
    score: float = None         # op "count": the score to count against
    expected: tuple = field(default=None, repr=False)

    @functools.cached_property
    def mask(self):
        return None if self.keep is None else oc.mask_from_bool(self.keep)

    @property
    def nq(self):
        return self.Q.shape[0]


@dataclass
class Palette:
    name: str
    n: int
    d: int
    A: np.ndarray = field(repr=False)
    index_kwargs: dict
    synth_seed: int = None      # the bulk comes from fill_synthetic(seed, n); None: upload(A)
    blocks: list = field(default_factory=list)   # planted (name, row0, rows) written with upload(rows, row0=row0)
    tag: np.ndarray = None      # the integer column of the predicate kinds
    kinds: list = field(default_factory=list)

    def populate(self, idx):
        if self.synth_seed is None:
            idx.upload(self.A)
        else:
            idx.fill_synthetic(self.synth_seed, self.n)
            for _, row0, rows in self.blocks:
                idx.upload(rows, row0=row0)

    def kind(self, name):
        return next(kd for kd in self.kinds if kd.name == name)

    def quiet_kinds(self):
        """The kinds whose host call never comes back flagged: a circuit of these alone keeps trying the short chain."""
        return [kd for kd in self.kinds if not kd.flags]


def _expect(pal, kd):
    """The oracle's answer in the shape the library returns it: rows / scores [nq, k] padded with NO_ROW / -inf, counts [nq]."""
    mask = kd.mask
    if kd.op == "count":
        s = oc.scores_all(pal.A, kd.Q[0], kd.metric, nthreads=8, native=True)
        return int(np.sum(s > F(kd.score))), int(np.sum(s == F(kd.score)))
    rows = np.full((kd.nq, kd.k), NO_ROW, np.uint64)
    scores = np.full((kd.nq, kd.k), -np.inf, F)
    counts = np.zeros(kd.nq, np.uint32)
    for i in range(kd.nq):
        er, es = oc.search(pal.A, kd.Q[i], kd.k, kd.metric, mask=mask, nthreads=8, partial=True, native=True)
        rows[i, :er.size], scores[i, :er.size], counts[i] = er, es, er.size
    return rows, scores, counts


def _finish(pal):
    for kd in pal.kinds:
        kd.Q = np.ascontiguousarray(np.atleast_2d(kd.Q), dtype=F)
        kd.expected = _expect(pal, kd)
    assert len({kd.name for kd in pal.kinds}) == len(pal.kinds)
    return pal


def _kth_score(pal, q, metric, kth):
    _, es = oc.search(pal.A, q, kth, metric, nthreads=8, partial=True, native=True)
    return float(es[-1])


def _palette_L():
    n, d, k = 270_000, 256, 20      # >= 4096 tiles (ring), >= 2^18 rows (crowd list, device-wide select), stride a multiple of 256 (8-bit sweeps)
    A = oc.synth(4242, 0, n, d, nthreads=8)
    Q = oc.synth(4243, 0, 8, d)
    rng = np.random.default_rng(3)
    keep40 = rng.random(n) < 0.4
    # 20 000 exact copies of one vector: far more ties at the top than the candidate capacity, few enough for the crowd list
    qc = oc.synth(4244, 0, 1, d)[0]
    crowd = np.tile((qc * F(1.5)).astype(F), (20_000, 1))
    # 6 000 rows within ~2e-4 in cosine of each other around another vector (relative noise 0.05, as in
    # test_bf16_pass_overflow_is_retried_in_f32, at the bulk's scale so that no kind's dot-product margin widens): the bf16 pass
    # overflows the candidate list; on a shard of this size the crowd list takes the 6 000 (fewer than an eighth of the rows)
    qr = oc.synth(4245, 0, 1, d)[0]
    near = (qr[None, :] + F(0.05) * F(qr.std()) * rng.standard_normal((6000, d))).astype(F)
    # 36 000 rows whose cosines to a third vector spread evenly over 1.5e-4 .. 1.8e-3 below 1: all of them within the bf16 mirror's
    # margin (2 rho_v >= 2.2e-3) of the 50th best, more than an eighth of the shard, so the crowd kernels decline; ~2 000 of them
    # within the f32 margin (2 * 3(d+10)u = 9.5e-5): the f32 retry sweep and its selection answer
    qf = oc.synth(4246, 0, 1, d)[0]
    amp = np.sqrt(rng.uniform(4e-4, 2.8e-3, 36_000)).astype(F)
    graded = (qf[None, :] + amp[:, None] * F(np.sqrt(np.mean(qf.astype(np.float64) ** 2))) * rng.standard_normal((36_000, d))).astype(F)
    blocks = [("crowd", 40_000, crowd), ("near", 150_000, near), ("graded", 200_000, graded)]
    for _, row0, rows in blocks:
        A[row0:row0 + rows.shape[0]] = rows
    sparse = np.zeros(n, bool)
    sparse[rng.choice(n, 12, replace=False)] = True     # fewer rows than k: survivor walk, count < k, padded tail
    tag = ((np.arange(n, dtype=np.uint64) * np.uint64(2654435761)) % np.uint64(1 << 32) % np.uint64(10_000)).astype(np.int64)
    pal = Palette("L", n, d, A, dict(single_launch=False), synth_seed=4242, blocks=blocks, tag=tag)
    S = "search"
    pal.kinds = [
        # the eight sweeps of test_every_sweep_reports_its_kind
        Kind("ring_f32", S, 0, Q[:1], k, COS, fp=("ring_f32", 4, 0)),
        Kind("valu_f32_bitmap", S, 0, Q[:1], k, L2, keep=keep40, fp=("valu_f32", 4, 0)),
        Kind("valu_f32_two", S, 0, Q[:2], k, DOT, fp=("valu_f32", 4, 0)),
        Kind("valu_bf16", S, 2, Q[1:2], k, COS, fp=("valu_bf16", 2, 0)),
        Kind("valu_i8", S, 1, Q[2:3], k, L2, fp=("valu_i8", 1, 0)),
        Kind("mfma_f32", S, 0, Q, k, DOT, fp=("mfma_f32", 4, 0)),
        Kind("mfma_bf16", S, 2, Q, k, L2, fp=("mfma_bf16", 2, 0)),
        Kind("mfma_i8", S, 1, Q, k, COS, fp=("mfma_i8", 1, 0)),
        Kind("sparse_bitmap", S, 1, Q[3:4], k, COS, keep=sparse, fp=("valu_i8", 1, 0)),
        Kind("crowd", S, 1, qc, 64, COS, fp=("valu_i8", 1, 0, True), crowd_min=20_000, flags=True),
        Kind("near_bf16", S, 2, qr, 50, COS, fp=("valu_bf16", 2, 0, True), crowd_min=6000, flags=True),
        Kind("retry_f32", S, 2, qf, 50, COS, fp=("valu_bf16", 2, 0, True), fits=True, flags=True),
        # k = the candidate capacity: any margin admits more rows than that, the query ends in the exact fallback + device-wide select
        Kind("k4096", S, 1, Q[4:5], 4096, DOT, fp=("valu_i8", 1, 1), flags=True),
        Kind("k5000_select_then_sort", S, 1, Q[5:6], 5000, L2, fp=("exact", 4, 0)),
        Kind("k200000_full_sort", S, 1, Q[6:7], 200_000, COS, fp=("exact", 4, 0)),
        Kind("pred_40pct", "pred", 1, Q[7:8], k, DOT, keep=tag < 4000, pred=("lt", 4000), fp=("valu_i8", 1, 0)),
        Kind("pred_few_rows", "pred", 2, Q[:1], 50, COS, keep=tag == 7, pred=("eq", 7), fp=("valu_bf16", 2, 0)),
    ]
    pal.kinds.append(Kind("count_exact", "count", 1, Q[:1], 1, L2, score=_kth_score(pal, Q[0], L2, 100)))
    return _finish(pal)


def _palette_T():
    n, d = 300_000, 32
    A, q = _corpora.identical_rows(n, d)
    keep1 = np.random.default_rng(31).random(n) < 0.01
    pal = Palette("T", n, d, A, dict())
    S = "search"
    Q3 = np.stack([q, q * F(2.0), -q]).astype(F)
    pal.kinds = [
        Kind("k10_cosine", S, 1, q, 10, COS, fp=("valu_bf16", 2, 1), flags=True),
        Kind("k10_euclidean", S, 1, q, 10, L2, fp=("valu_bf16", 2, 1), flags=True),
        Kind("k10_dot", S, 1, q, 10, DOT, fp=("valu_bf16", 2, 1), flags=True),
        Kind("k4096", S, 1, q, 4096, COS, fp=("valu_bf16", 2, 1), flags=True),
        # (~3 000 selected rows fit the candidate list: the one kind of this palette that the candidate path answers)
        Kind("bitmap_1pct", S, 1, q, 50, L2, keep=keep1, fp=("valu_bf16", 2, 0)),
        Kind("three_queries", S, 1, Q3, 10, DOT, fp=("valu_bf16", 2, 3), flags=True),
        # the large-k path borrows the histogram and the barrier of the device-wide select that ran one call earlier / runs one later
        Kind("k6000_select_then_sort", S, 1, q, 6000, COS, fp=("exact", 4, 0)),
        Kind("k_all_rows", S, 1, q, n, L2, fp=("exact", 4, 0)),
    ]
    pal.kinds.append(Kind("count_exact", "count", 1, q, 1, DOT, score=_kth_score(pal, q, DOT, 1)))
    return _finish(pal)


def _palette_S():
    rng = np.random.default_rng(12)
    n, d = 6000, 16
    A = rng.standard_normal((n, d)).astype(F)
    A[1000:5500] = A[1000]                    # 4500 duplicates: a query near them overflows the candidate capacity
    Q = np.stack([A[1000] + 0.0, rng.standard_normal(d).astype(F), -A[1000]])
    keep40 = rng.random(n) < 0.4
    keep3 = np.zeros(n, bool)
    keep3[[17, 1000, 5999]] = True
    Q65 = rng.standard_normal((65, d)).astype(F)
    Q65[[0, 31, 64]] = [A[1000], A[1000] * F(2.0), -A[1000]]
    # a default index: tiny_search_kernel serves lone small calls.  (Below 2^18 rows the host API has no short chain: no kind "flags".)
    pal = Palette("S", n, d, A, dict())
    S = "search"
    pal.kinds = [
        Kind("lone_k5", S, 1, Q[1], 5, COS, fp=("exact", 4, 0)),                       # one launch
        Kind("lone_k5_duplicates", S, 1, Q[0], 5, DOT, fp=("exact", 4, 0)),            # one launch, 4500 ties at the top
        Kind("lone_k2000", S, 1, Q[1], 2000, L2, fp=("valu_bf16", 2, 1)),              # the general chain; k reaches into the duplicates
        Kind("mixed_three", S, 1, Q, 5, COS, fp=("valu_bf16", 2, 1)),                  # fallback queries beside normal ones
        Kind("bitmap_40pct", S, 1, Q[1], 5, DOT, keep=keep40, fp=("valu_bf16", 2, 0)),
        Kind("bitmap_3_rows", S, 1, Q[0], 5, COS, keep=keep3, fp=("valu_bf16", 2, 0)),
        Kind("k5000", S, 1, Q[1], 5000, COS, fp=("exact", 4, 0)),
        Kind("k_beyond_rows", S, 1, Q[1], n + 1000, DOT, fp=("exact", 4, 0)),
        Kind("batch_65", S, 1, Q65, 5, L2, fp=("valu_bf16", 2, 2)),
    ]
    return _finish(pal)


@functools.lru_cache(maxsize=None)
def palette(name):
    """The palette and its oracle answers, built once per process and shared by every test (read only)."""
    return {"L": _palette_L, "T": _palette_T, "S": _palette_S}[name]()


def pred_program(kd, column):
    """The predicate program of a "pred" kind on GpuColumns column `column`."""
    cmp_, value = kd.pred
    return [(_capi.PRED_CMP, {"lt": _capi.CMP_LT, "eq": _capi.CMP_EQ}[cmp_], _capi.CELL_INT, column, int(value), 0)]


def expected_shape_problems(pal, kd):
    """What is wrong with a kind's expected answer given its k and bitmap ([] = nothing): the CPU test's check."""
    bad = []
    if kd.op == "count":
        gt, eq = kd.expected
        if not (0 <= gt and 1 <= eq and gt + eq <= pal.n):
            bad.append(f"count_exact expects {gt} above, {eq} equal of {pal.n}")
        return bad
    rows, scores, counts = kd.expected
    want = min(kd.k, pal.n if kd.keep is None else int(kd.keep.sum()))
    if rows.shape != (kd.nq, kd.k) or scores.shape != (kd.nq, kd.k) or counts.shape != (kd.nq,):
        bad.append(f"shapes {rows.shape} {scores.shape} {counts.shape}")
    for i in range(kd.nq):
        c = int(counts[i])
        if c != want:
            bad.append(f"query {i}: count {c}, k and bitmap imply {want}")
        if not (np.all(rows[i, c:] == NO_ROW) and np.all(np.isneginf(scores[i, c:]))):
            bad.append(f"query {i}: tail not padded")
        if np.any(rows[i, :c] >= pal.n) or np.unique(rows[i, :c]).size != c:
            bad.append(f"query {i}: rows out of range or repeated")
        if kd.keep is not None and not np.all(kd.keep[rows[i, :c].astype(np.int64)]):
            bad.append(f"query {i}: a row the bitmap excludes")
        s = scores[i, :c]
        if np.any(np.isnan(s)) or np.any(s[1:] > s[:-1]):
            bad.append(f"query {i}: scores not descending")
    return bad


def mismatch(kd, got):
    """None if `got` — (rows u64 [nq,k], scores f32 [nq,k], counts [nq]) or count_exact's (above, equal) — is the kind's expected
    answer in every slot (rows, score BITS, counts, the padded tail), else a short description."""
    if kd.op == "count":
        return None if tuple(int(x) for x in got) == kd.expected else f"count_exact {tuple(got)} != {kd.expected}"
    rows, scores, counts = got
    er, es, ec = kd.expected
    rows = np.asarray(rows).view(np.uint64).reshape(er.shape)
    scores = np.asarray(scores, dtype=F).reshape(es.shape)
    counts = np.asarray(counts).view(np.uint32).reshape(ec.shape)
    if not np.array_equal(counts, ec):
        return f"counts {counts[:8]} != {ec[:8]}"
    for i in range(kd.nq):
        c = int(ec[i])
        if not np.array_equal(rows[i, :c], er[i, :c]):
            j = int(np.flatnonzero(rows[i, :c] != er[i, :c])[0])
            return f"query {i}: rows differ first at slot {j}: {rows[i, j]} != {er[i, j]}"
        if not np.array_equal(scores[i, :c].view(np.uint32), es[i, :c].view(np.uint32)):
            j = int(np.flatnonzero(scores[i, :c].view(np.uint32) != es[i, :c].view(np.uint32))[0])
            return f"query {i}: score bits differ first at slot {j}: {scores[i, j]!r} != {es[i, j]!r}"
        if not (np.all(rows[i, c:] == NO_ROW) and np.all(np.isneginf(scores[i, c:]))):
            return f"query {i}: the tail behind slot {c} is not NO_ROW / -inf"
    return None
