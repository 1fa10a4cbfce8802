"""The cases of the top-k search over a delta set (docs/delta.md §8), shared by tests/test_deltaset_cpu.py (the library's host path,
min_device_rows = NEVER) and tests/test_gpu_deltaset.py (the device path, min_device_rows = 0).  Every check holds rows, score bits
and counts to the twin tests/_deltaset_oracle.py bit for bit, a NaN compared as a NaN.

Planting scores (docs/delta.md §1, Sums): against a zero archetype and the query e0, a row of the one entry (0, d) scores
+0.0 + (-0.0 + d * 1) = d exactly (d = -0.0 gives +0.0), so a test places any f32 pattern but -0.0; a -0.0 comes from a row of no
entries under an all-negative query.  The twin computes every expected score all the same; the rule only chooses the inputs.

The shapes: n around the wave (63, 64, 65), around 1024 rows (one row per thread of the select workgroup), around its step of 4096
rows (four per thread: 4095, 4096, 4097) and past two steps; k at 1, 2, n - 1, n, n + 1; k at the select kernel's last and the
large-k path's first (4096, 4097 on 5000 rows)."""
import threading

import numpy as np

from tests import _delta_cases as dc
from tests import _delta_oracle as do
from tests import _deltaset_oracle as dso

F = np.float32
SIZES = (1, 63, 64, 65, 1023, 1024, 1025, 2049, 4095, 4096, 4097)
DIM = 2
E0 = np.asarray([1.0, 0.0], dtype=F)
NEGATIVE = np.asarray([-1.0, -1.0], dtype=F)
METRICS = ("dot", "cosine")
_CACHE = {}


def from_bits(words):
    return np.asarray(words, dtype=np.uint32).view(F)


def planted(mdr, values, empty=()):
    """-> (the library's set, the twin's registry, the twin's rows): row i holds the one entry (0, values[i]), or none if i is in
    `empty`, against the zero archetype"""
    values = np.asarray(values, dtype=F)
    lib, twin = dc.registries(DIM, np.zeros((1, DIM)), mdr=mdr)
    gone = set(int(i) for i in empty)
    deltas = [do.DeltaVector(0, DIM, [], []) if i in gone else do.DeltaVector(0, DIM, [0], values[i:i + 1]) for i in range(len(values))]
    return dc.lib_set(lib, deltas), twin, deltas


def expect(twin, deltas, queries, metric, tag=None):
    """the twin's scores [nq][n], computed once per tag and left unchanged"""
    if tag is None:
        return dso.scores_of(twin, deltas, queries, metric)
    key = (tag, metric)
    if key not in _CACHE:
        _CACHE[key] = dso.scores_of(twin, deltas, queries, metric)
        _CACHE[key].setflags(write=False)
    return _CACHE[key]


def assert_answer(got, scores, k, what=""):
    rows, sc, counts = got
    w_rows, w_sc, w_counts = dso.top_k_all(scores, k)
    assert rows.dtype == np.int64 and rows.shape == w_rows.shape and sc.shape == w_sc.shape, what
    assert np.array_equal(counts, w_counts), (what, counts, w_counts)
    bad = np.argwhere(rows != w_rows)
    assert bad.size == 0, (what, k, bad[:4].tolist(), rows[tuple(bad[0])], w_rows[tuple(bad[0])])
    assert dc.same(sc, w_sc), (what, k)


def check(s, twin, deltas, queries, ks, metrics=METRICS, tag=None):
    """-> the twin's scores under the first of `metrics`"""
    for metric in metrics:
        scores = expect(twin, deltas, queries, metric, tag)
        for k in ks:
            assert_answer(s.search(queries, k, metric), scores, k, (tag, metric))
    return expect(twin, deltas, queries, metrics[0], tag)


def mixed_values(n, seed):
    """both signs, many ties (a pool of 23 values, zero among them) and a few rows of their own"""
    rng = np.random.default_rng(seed + n)
    pool = np.concatenate([rng.standard_normal(22).astype(F) * F(3.0), [F(0.0)]])
    v = pool[rng.integers(0, pool.size, size=n)].astype(F)
    own = rng.permutation(n)[:max(1, n // 5)]
    v[own] = rng.standard_normal(own.size).astype(F)
    return v


# ---- sizes and k ----------------------------------------------------------------------------------------------------------------

def check_sizes(mdr, n):
    s, twin, deltas = planted(mdr, mixed_values(n, 100))
    ks = sorted({k for k in (1, 2, n - 1, n, n + 1) if k >= 1})
    q = np.stack([E0, NEGATIVE])
    scores = check(s, twin, deltas, q, ks, tag=("sizes", n))
    assert dc.same(scores[0], [d.deltas[0] + F(0.0) for d in deltas])          # the planting rule holds: the dot is d
    rows, sc, counts = s.search(q, n + 1)
    assert counts.tolist() == [n, n] and (rows[:, n] == dso.NO_ROW).all() and np.isneginf(sc[:, n]).all()


def check_k_border(mdr, k):
    """5000 rows: k = 4096 is the select kernel's last, 4097 the large-k path's first; the cosines are +-1 and 0, ties by the thousand"""
    n = 5000
    s, twin, deltas = planted(mdr, mixed_values(n, 200))
    check(s, twin, deltas, np.stack([E0, NEGATIVE]), (k,), tag=("border", n))
    if k > 4096:
        check(s, twin, deltas, np.stack([E0, NEGATIVE]), (n, n + 3), metrics=("dot",), tag=("border", n))


# ---- ties -----------------------------------------------------------------------------------------------------------------------

def check_all_equal(mdr):
    n = 4500
    s, twin, deltas = planted(mdr, np.full(n, 2.5, dtype=F))
    scores = check(s, twin, deltas, E0[None, :], (1, 2, 64, 65, 1025, 4096, n - 1, n), metrics=("dot",), tag="all equal")
    assert (dc.bits(scores) == dc.bits(F(2.5))).all()
    rows, _, _ = s.search(E0, 1025)
    assert rows[0].tolist() == list(range(1025))


def tie_run_values(n, runs, head):
    v = np.full(n, 1.0, dtype=F)
    v[:head] = 5.0
    for b, e in runs:
        v[b:e] = 2.0
    return v


def check_tie_runs(mdr):
    """60 rows above a run of equal scores whose members sit on both sides of rows 63 / 64, 1023 / 1024 and 4095 / 4096: every cut
    from the run's first member to one past its last"""
    n, head, runs = 4200, 60, ((61, 67), (1021, 1027), (4093, 4099))
    s, twin, deltas = planted(mdr, tie_run_values(n, runs, head))
    members = sum(e - b for b, e in runs)
    ks = list(range(head, head + members + 2))
    scores = check(s, twin, deltas, E0[None, :], ks, metrics=("dot",), tag="tie runs")
    rows, _, _ = dso.top_k_all(scores, head + 9)
    assert rows[0, head:].tolist() == [61, 62, 63, 64, 65, 66, 1021, 1022, 1023]            # the cut falls between 1023 and 1024
    rows, _, _ = s.search(E0, head + 15)
    assert rows[0, head:].tolist() == [61, 62, 63, 64, 65, 66, 1021, 1022, 1023, 1024, 1025, 1026, 4093, 4094, 4095]


def check_zeros(mdr):
    """+0.0 beside -0.0 under the all-negative query: a row of no entries scores -0.0 + -0.0 = -0.0, a row (0, 0.0) as well, a row
    (0, -0.0) scores +0.0; they tie, the row decides, and each answer carries its own bits"""
    n = 200
    v = np.zeros(n, dtype=F)
    v[1::3] = F(-0.0)
    v[5::7] = F(1.0)                                    # scores of -1.0 below the zeros
    v[6::11] = F(-2.0)                                  # and of 2.0 above them
    empty = range(0, n, 4)
    s, twin, deltas = planted(mdr, v, empty)
    scores = check(s, twin, deltas, NEGATIVE[None, :], (1, 2, 50, 100, 150, n), metrics=("dot",), tag="zeros")
    zero = scores[0] == 0
    assert {0x80000000, 0} == set(dc.bits(scores[0][zero]).tolist()) and 40 < zero.sum() < n
    rows, sc, _ = s.search(NEGATIVE, 150)
    picked = rows[0][sc[0] == 0]
    assert (np.diff(picked) > 0).all() and len(set(dc.bits(sc[0][sc[0] == 0]).tolist())) == 2
    assert np.array_equal(dc.bits(sc[0]), dc.bits(scores[0][rows[0]]))


# ---- special scores ---------------------------------------------------------------------------------------------------------------

def check_specials(mdr):
    n = 1100
    v = mixed_values(n, 300)
    v[3::17] = np.nan
    v[[5, 700]] = from_bits([0x7FC12345, 0xFFC00001])                                       # NaNs with payloads, either sign
    v[[8, 1030]] = np.inf
    v[[9, 64, 1024]] = -np.inf
    s, twin, deltas = planted(mdr, v)
    finite = int((~np.isnan(v)).sum())
    scores = check(s, twin, deltas, E0[None, :], (1, 2, 3, finite - 1, finite, finite + 1, finite + 5, n, n + 2), metrics=("dot",),
                   tag="specials")
    rows, sc, _ = s.search(E0, n)
    assert rows[0, :2].tolist() == [8, 1030] and np.isnan(sc[0, finite:]).all() and not np.isnan(sc[0, :finite]).any()
    assert rows[0, finite - 3:finite].tolist() == [9, 64, 1024]                             # -inf is above every NaN
    assert (np.diff(rows[0, finite:]) > 0).all()                                            # the NaNs tie: by row
    own = s.dot_dense(E0)[0]
    assert np.array_equal(dc.bits(sc[0]), dc.bits(own[rows[0]]))                            # a NaN's payload is the row's own    # every score NaN: rows 0 .. k - 1
    s2, twin2, deltas2 = planted(mdr, np.full(300, np.nan, dtype=F))
    check(s2, twin2, deltas2, E0[None, :], (1, 64, 65, 300, 301), metrics=("dot",), tag="all nan")
    assert s2.search(E0, 70)[0][0].tolist() == list(range(70))
    # a zero query: every cosine is 0.0, no special case
    s3, twin3, deltas3 = planted(mdr, mixed_values(130, 301))
    check(s3, twin3, deltas3, np.zeros((1, DIM), dtype=F), (1, 5, 130, 131), tag="zero query")
    rows, sc, _ = s3.search(np.zeros(DIM, dtype=F), 5, "cosine")
    assert rows[0].tolist() == [0, 1, 2, 3, 4] and (dc.bits(sc) == 0).all()


# ---- the three radix passes ---------------------------------------------------------------------------------------------------------

def radix_values(which):
    rng = np.random.default_rng(400)
    if which == "low":                                   # scores that differ in bits 9-0 only: the third pass decides
        words = np.uint32(0x3F800000) + rng.integers(0, 1024, size=1500).astype(np.uint32)
    elif which == "mid":                                 # in bits 20-10 only: the second pass decides
        words = np.uint32(0x3F800000) + (rng.integers(0, 2048, size=2500).astype(np.uint32) << np.uint32(10))
    else:                                                # every combination of the top 11 bits once, exponent 255 left out
        top = np.asarray([t for t in range(2048) if (t >> 2) & 0xFF != 0xFF], dtype=np.uint32)
        words = (rng.permutation(top) << np.uint32(21)) | np.uint32(0x00012345)
    return from_bits(words)


def check_radix(mdr, which):
    v = radix_values(which)
    n = len(v)
    s, twin, deltas = planted(mdr, v)
    scores = check(s, twin, deltas, E0[None, :], (1, 2, 7, 64, 500, 1024, n - 1, n), metrics=("dot",), tag=("radix", which))
    assert np.array_equal(dc.bits(scores[0]), dc.bits(v))                                   # every pattern arrives as planted
    keys = dso.score_to_key(v)
    if which == "low":
        assert len(set((keys >> 10).tolist())) == 1 and len(set(keys.tolist())) > 700
    elif which == "mid":
        assert len(set((keys >> 21).tolist())) == 1 and len(set((keys & 1023).tolist())) == 1 and len(set(keys.tolist())) > 1400
    else:
        assert len(set((keys >> 21).tolist())) == n


# ---- real sets ----------------------------------------------------------------------------------------------------------------------

def check_scored_set(mdr, nq):
    """the 130 rows of the score tests (four archetypes, cached and computed magnitudes, inf and NaN in the queries)"""
    arch, twin, deltas = dc.score_inputs()
    lib, _ = dc.registries(arch.shape[1], arch, mdr=mdr)
    s = dc.lib_set(lib, deltas)
    q = dc.score_queries(arch.shape[1], nq)
    check(s, twin, deltas, q, (1, 7, 129, 130, 131), tag=("scored", nq))


def check_encoded_and_unsorted(mdr):
    """a set from encode_batch beside a from_parts set with unsorted and repeated positions"""
    arch, rows = dc.encode_inputs(65, n=70)
    lib, twin = dc.registries(65, arch, mdr=mdr)
    q = dc.score_queries(65, 2)
    for with_magnitude in (False, True):
        s = lib.encode_batch(rows, 1e-3, with_magnitude)
        want = [d for d, _ in twin.encode_batch(rows, 1e-3, with_magnitude)]
        check(s, twin, want, q, (1, 10, 70, 71), tag=("encoded", with_magnitude))
    arch, twin, deltas = dc.parts_inputs()
    lib, _ = dc.registries(arch.shape[1], arch, mdr=mdr)
    s = dc.lib_set(lib, deltas)
    assert not s.arrays()["sorted"].all()
    check(s, twin, deltas, np.random.default_rng(4).standard_normal((2, arch.shape[1])).astype(F), (1, 9, len(deltas)), tag="unsorted")


def check_empty_set_and_refusals(mdr):
    from neumann_amd import DeltaSet, DeltaVectorError
    lib, _ = dc.registries(DIM, np.zeros((1, DIM)), mdr=mdr)
    s = DeltaSet.from_parts(lib, [], [0], [], [])
    rows, sc, counts = s.search(np.stack([E0, NEGATIVE]), 3)
    assert counts.tolist() == [0, 0] and (rows == dso.NO_ROW).all() and np.isneginf(sc).all() and rows.shape == (2, 3)
    one, _, _ = planted(mdr, [1.0])
    for call, text in ((lambda: one.search(E0, 0), "a top-k search needs k of at least 1"),
                       (lambda: one.search(E0, 1, "euclidean"), "metric must be"),
                       (lambda: one.search(np.ones(3), 1), "must be [n][2]")):
        try:
            call()
        except DeltaVectorError as e:
            assert text in str(e), str(e)
        else:
            raise AssertionError(f"not refused: {text}")
    assert one.search(np.zeros((0, DIM)), 4)[0].shape == (0, 4)


def check_query_blocks(mdr):
    """more queries than one block of the host-buffer form takes: 70 000 rows x 1000 queries are 280 MB of score words against the
    budget of 256 MiB.  The queries are c * e0 with c a power of two, so the score of row i is c * d_i exactly; the rule is held to
    the twin on the first rows, the answers to the order on every query"""
    from neumann_amd import DeltaSet, delta
    n, nq, k = 70000, 1000, 3
    assert n * 4 * nq > delta.search_limits()[2] >= n * 4
    rng = np.random.default_rng(500)
    v = rng.standard_normal(n).astype(F)
    lib, twin = dc.registries(DIM, np.zeros((1, DIM)), mdr=mdr)
    s = DeltaSet.from_parts(lib, np.zeros(n, dtype=np.uint64), np.arange(n + 1), np.zeros(n, dtype=np.uint16), v)
    c = (F(2.0) ** rng.integers(-3, 4, size=nq).astype(F)) * rng.choice([-1.0, 1.0], size=nq).astype(F)
    q = np.zeros((nq, DIM), dtype=F)
    q[:, 0] = c
    head = [do.DeltaVector(0, DIM, [0], v[i:i + 1]) for i in range(40)]
    assert dc.same(dso.scores_of(twin, head, q[:5], "dot"), c[:5, None] * v[None, :40])
    rows, sc, counts = s.search(q, k)
    assert (counts == k).all()
    for i in (0, 1, 2, 500, 957, 958, 959, 998, 999):      # the borders of the blocks of 958 queries, whatever the block is
        w_rows, w_sc, _ = dso.top_k(c[i] * v, k)
        assert np.array_equal(rows[i], w_rows) and dc.same(sc[i], w_sc), i
    best = np.where(c > 0, v.max(), -v.min()) * np.abs(c)
    assert dc.same(sc[:, 0], best.astype(F))


def check_single_query_threshold(mdr):
    """a single query over 2^18 rows or more is ranked by the sort of the large-k path, one row fewer or a second query by the select
    kernel (delta.search_limits()[3]): the same answers on both sides of it.  Scores planted as in check_query_blocks."""
    from neumann_amd import DeltaSet, delta
    edge = delta.search_limits()[3]
    assert edge == 1 << 18
    rng = np.random.default_rng(600)
    pool = rng.standard_normal(5000).astype(F)
    for n in (edge - 1, edge):
        v = pool[rng.integers(0, pool.size, size=n)]                                         # ties by the dozen
        lib, twin = dc.registries(DIM, np.zeros((1, DIM)), mdr=mdr)
        s = DeltaSet.from_parts(lib, np.zeros(n, dtype=np.uint64), np.arange(n + 1), np.zeros(n, dtype=np.uint16), v)
        q = np.zeros((2, DIM), dtype=F)
        q[:, 0] = (2.0, -0.5)
        head = [do.DeltaVector(0, DIM, [0], v[i:i + 1]) for i in range(40)]
        assert dc.same(dso.scores_of(twin, head, q, "dot"), q[:, :1] * v[None, :40])
        scores = q[:, :1] * v[None, :]
        for k in (1, 10, 4096):
            assert_answer(s.search(q[:1], k), scores[:1], k, (n, k, "one query"))
            assert_answer(s.search(q, k), scores, k, (n, k, "two queries"))


# ---- concurrency and history --------------------------------------------------------------------------------------------------------

def check_two_threads(mdr):
    arch, twin, deltas = dc.score_inputs()
    lib, _ = dc.registries(arch.shape[1], arch, mdr=mdr)
    s = dc.lib_set(lib, deltas)
    q = dc.score_queries(arch.shape[1], 5)
    want = {m: expect(twin, deltas, q, m, ("scored", 5)) for m in METRICS}
    results, errors = {}, []

    def work(name):
        try:
            for _ in range(3):
                results[name] = (s.search(q, 9, "dot"), s.search(q, 131, "cosine"), s.dot_dense(q))
        except Exception as e:      # noqa: BLE001
            errors.append(e)
    threads = [threading.Thread(target=work, args=(i,)) for i in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    assert len(results) == 2
    for r in results.values():
        assert_answer(r[0], want["dot"], 9)
        assert_answer(r[1], want["cosine"], 131)
        assert dc.same(r[2], want["dot"])


def check_history(mdr):
    """an answer does not depend on the calls before it: other k, the other metric, the large-k path, the scores, another set"""
    n = 5000
    s, twin, deltas = planted(mdr, mixed_values(n, 200))
    q = np.stack([E0, NEGATIVE])
    scores = expect(twin, deltas, q, "dot", ("border", n))
    first = s.search(q, 10)
    assert_answer(first, scores, 10)
    s.search(q, 4097), s.search(q[:1], 4096, "cosine"), s.dot_dense(q), s.to_dense()
    other, _, _ = planted(mdr, mixed_values(300, 7))
    other.search(E0, 300)
    again = s.search(q, 10)
    assert all(np.array_equal(a, b) for a, b in zip(first[:1] + first[2:], again[:1] + again[2:])) and dc.same(first[1], again[1])
    assert_answer(s.search(q[1:], 1), scores[1:], 1)


# ---- sets made on the device (docs/delta.md §9; these need a GPU) -------------------------------------------------------------------

def device_registries(dim, arch, **kw):
    lib, twin = dc.registries(dim, arch, mdr=dc.ALWAYS, **kw)
    return lib.to_device(), twin


def encode_device(lib, rows, threshold, with_magnitude=False, **kw):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(rows, dtype=F)).cuda()
    torch.cuda.synchronize()
    return lib.encode_batch_device(t, threshold, with_magnitude, **kw)


def assert_device_born(s, lib, twin, want, queries):
    """a set without host arrays against the twin's rows: the stored counts, the magnitudes, scores and search against the from_parts
    set of the same content — none of which brings the arrays to the host — and then every array"""
    assert not s.host_arrays_present and len(s) == len(want) and s.nnz == sum(d.nnz() for d in want)
    same_content = dc.lib_set(lib, want)
    assert dc.same(s.magnitudes(), do.magnitudes(twin, want))
    for a, b in ((s.dot_dense(queries), same_content.dot_dense(queries)),
                 (s.cosine_similarity_dense(queries), same_content.cosine_similarity_dense(queries))):
        assert dc.same(a, b)
    assert dc.same(s.dot_dense(queries), do.dot_dense_all(twin, want, queries))
    for metric in METRICS:
        got, ref = s.search(queries, 7, metric), same_content.search(queries, 7, metric)
        assert np.array_equal(got[0], ref[0]) and dc.same(got[1], ref[1]) and np.array_equal(got[2], ref[2])
    assert dc.same(s.to_dense(), do.decode_all(twin, want))
    assert not s.host_arrays_present
    dc.assert_set_equals(s, want)
    assert s.host_arrays_present and s.arrays()["sorted"].all()
    if not any(d.cached_magnitude is not None for d in want):
        a = s.arrays()
        assert (dc.bits(a["cached_magnitudes"]) == 0).all() and not a["has_cached"].any()


def check_encode_device(dim, threshold):
    arch, rows = dc.encode_inputs(dim)
    lib, twin = device_registries(dim, arch)
    q = dc.score_queries(dim, 2)
    for with_magnitude in (False, True):
        s = encode_device(lib, rows, threshold, with_magnitude)
        want = [d for d, _ in twin.encode_batch(rows, threshold, with_magnitude)]
        assert_device_born(s, lib, twin, want, q)


def check_encode_device_rows(n):
    """n around the wave and the slice (1, 63, 64, 65, 130), past the old scan's block (300) and past the new scan's (1100)"""
    arch, rows = dc.encode_inputs(65, n=max(n, 8))
    rows = rows[:n]
    lib, twin = device_registries(65, arch)
    s, ids, sims = encode_device(lib, rows, 1e-3, n % 2 == 0, return_assignments=True)
    w_ids, w_sims = twin.find_best_many(rows)
    assert np.array_equal(ids.cpu().numpy(), w_ids) and dc.same(sims.cpu().numpy(), w_sims)
    assert_device_born(s, lib, twin, [d for d, _ in twin.encode_batch(rows, 1e-3, n % 2 == 0)], dc.score_queries(65, 2))


def check_encode_device_slices():
    """257 full slices and one row at 8 dimensions (16 449 rows: the slice scan of the issue's 256 block and a partial last slice),
    against the twin; 1025 slices and one row (65 601 rows: past the 1024 of the scan that is used), against the host path, which
    the other tests hold to the twin; a slice of only empty rows between two full ones (two slices share an offset)"""
    rng = np.random.default_rng(700)
    arch = rng.standard_normal((3, 8)).astype(F)
    lib, twin = device_registries(8, arch)
    q = rng.standard_normal((2, 8)).astype(F)
    for n, against_twin in ((16449, True), (65601, False)):
        rows = arch[rng.integers(0, 3, size=n)] + (rng.random((n, 8)) < 0.4) * rng.standard_normal((n, 8)).astype(F)
        rows = rows.astype(F)
        s = encode_device(lib, rows, 1e-3, False)
        assert not s.host_arrays_present
        dot, mags, top = s.dot_dense(q), s.magnitudes(), s.search(q, 5)
        if against_twin:
            want = [d for d, _ in twin.encode_batch(rows, 1e-3, False)]
            dc.assert_set_equals(s, want)
            assert dc.same(dot, do.dot_dense_all(twin, want, q)) and dc.same(mags, do.magnitudes(twin, want))
        lib.set_min_device_rows(dc.NEVER)
        h = lib.encode_batch(rows, 1e-3, False)
        ha, sa = h.arrays(), s.arrays()
        assert all(np.array_equal(ha[k], sa[k]) for k in ("archetype_ids", "indptr", "positions", "has_cached", "sorted"))
        assert dc.same(ha["deltas"], sa["deltas"]) and dc.same(ha["cached_magnitudes"], sa["cached_magnitudes"])
        assert dc.same(dot, h.dot_dense(q)) and dc.same(mags, h.magnitudes())
        ht = h.search(q, 5)
        assert np.array_equal(top[0], ht[0]) and dc.same(top[1], ht[1])
        lib.set_min_device_rows(dc.ALWAYS)
    rows = np.repeat(arch[:1], 192, axis=0)
    rows[:64] += F(1.0)
    rows[128:] -= F(2.0)
    s = encode_device(lib, rows, 0.0, True)
    want = [d for d, _ in twin.encode_batch(rows, 0.0, True)]
    assert [d.nnz() for d in want] == [8] * 64 + [0] * 64 + [8] * 64
    assert_device_born(s, lib, twin, want, q)


def check_encode_device_wide():
    """one row at dimension 65535 whose last position is kept; 65536 refused with the reference's text"""
    from neumann_amd import DeltaVectorError
    dim = do.MAX_DIMENSION
    arch = np.zeros((2, dim), dtype=F)
    arch[0, ::7], arch[1, ::5] = 1.0, -1.0
    row = arch[0].copy()
    row[dim - 1] += 3.0
    row[1000] -= 2.0
    lib, twin = device_registries(dim, arch)
    s = encode_device(lib, row[None, :], 0.5, True)
    dc.assert_set_equals(s, [twin.encode(row, 0.5, True)])
    assert s.positions.tolist() == [1000, dim - 1]
    lib2, _ = device_registries(dim + 1, np.zeros((1, dim + 1)))
    try:
        encode_device(lib2, np.zeros((1, dim + 1)), 0.5)
    except DeltaVectorError as e:
        assert str(e) == do.dimension_exceeded(dim + 1) == "dimension 65536 exceeds maximum 65535 (u16::MAX)"
    else:
        raise AssertionError("a dimension of 65536 was not refused")


def check_host_arrays_on_first_need():
    """no host copy after encode_batch_device nor after the host-buffer encode_batch on its device path, none after scores and a
    search, one after arrays(); two threads asking together get one set of arrays; after min_device_rows = never every operation
    answers from the downloaded arrays with the same bits"""
    arch, rows = dc.encode_inputs(65, n=130)
    lib, twin = device_registries(65, arch)
    q = dc.score_queries(65, 2)
    want = [d for d, _ in twin.encode_batch(rows, 1e-3, False)]
    for s in (encode_device(lib, rows, 1e-3, False), lib.encode_batch(rows, 1e-3, False)):
        assert not s.host_arrays_present
        n = len(want)
        pairs = [(i, (i * 7 + 3) % n) for i in range(n)]
        dev = [s.dot_dense(q), s.cosine_similarity_dense(q), s.to_dense(), s.magnitudes(), lib.dot_deltas_same_archetype(s, s, pairs)[0]]
        top = s.search(q, 9, "cosine")
        assert not s.host_arrays_present and s.nnz == sum(d.nnz() for d in want)
        results = []
        threads = [threading.Thread(target=lambda: results.append(s.arrays())) for _ in range(2)]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
        assert s.host_arrays_present and len(results) == 2
        assert all(np.array_equal(results[0][k], results[1][k]) for k in ("indptr", "positions", "archetype_ids"))
        dc.assert_set_equals(s, want)
        lib.set_min_device_rows(dc.NEVER)
        host = [s.dot_dense(q), s.cosine_similarity_dense(q), s.to_dense(), s.magnitudes(), lib.dot_deltas_same_archetype(s, s, pairs)[0]]
        htop = s.search(q, 9, "cosine")
        lib.set_min_device_rows(dc.ALWAYS)
        assert all(dc.same(a, b) for a, b in zip(dev, host))
        assert np.array_equal(top[0], htop[0]) and dc.same(top[1], htop[1])
        assert dc.same(dev[0], do.dot_dense_all(twin, want, q)) and dc.same(dev[3], do.magnitudes(twin, want))
    # a device-born set that meets the host path FIRST: the download happens there
    s = encode_device(lib, rows, 1e-3, True)
    lib.set_min_device_rows(dc.NEVER)
    assert not s.host_arrays_present
    assert dc.same(s.dot_dense(q), do.dot_dense_all(twin, want, q)) and s.host_arrays_present
    host_born = dc.lib_set(lib, want)
    assert host_born.host_arrays_present


def check_encode_device_stream_and_refusals():
    import torch
    from neumann_amd import DeltaVectorError
    arch, rows = dc.encode_inputs(65, n=130)
    lib, twin = dc.registries(65, arch[:2], max_archetypes=3, mdr=dc.ALWAYS)
    t = torch.from_numpy(rows).cuda()
    torch.cuda.synchronize()
    empty, _ = dc.registries(65, np.zeros((0, 65)), max_archetypes=2, mdr=dc.ALWAYS)
    for reg, text in ((empty.to_device(), "the registry is empty"), (lib, "not resident")):
        try:
            reg.encode_batch_device(t, 1e-3)
        except DeltaVectorError as e:
            assert text in str(e), str(e)
        else:
            raise AssertionError(f"not refused: {text}")
    lib.to_device()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        s1 = lib.encode_batch_device(t, 1e-3, True)
    s2 = lib.encode_batch_device(t, 1e-3, False, stream=side.cuda_stream)
    want = {wm: [d for d, _ in twin.encode_batch(rows, 1e-3, wm)] for wm in (True, False)}
    q = dc.score_queries(65, 2)
    assert_device_born(s1, lib, twin, want[True], q)       # the library's own calls wait for the set's event
    assert_device_born(s2, lib, twin, want[False], q)
    assert len(lib.encode_batch_device(t[:0], 1e-3)) == 0
    assert lib.register(arch[2]) == 2                      # grown since: the mirror is not current
    try:
        lib.encode_batch_device(t, 1e-3)
    except DeltaVectorError as e:
        assert "not resident" in str(e) and "after the last register" in str(e), str(e)
    else:
        raise AssertionError("a registry grown since was not refused")


def check_encode_batch_joins_its_chunks():
    """the host-buffer encode_batch takes its rows up 256 MiB at a time: 1100 rows at dimension 65535 are two chunks (1024 + 76
    rows), whose CSR pieces are joined device to device.  Held to the host path, which the other tests hold to the twin."""
    dim, n = do.MAX_DIMENSION, 1100
    rng = np.random.default_rng(800)
    arch = np.zeros((2, dim), dtype=F)
    arch[0, ::7], arch[1, ::5] = 1.0, -1.0
    rows = arch[np.arange(n) % 2].copy()
    for i in range(n):
        rows[i, rng.integers(0, dim, size=i % 40)] += F(1.0)
    rows[1023, dim - 1] = 9.0
    rows[1024, 0] = 9.0                                  # the rows on either side of the chunk border
    lib, _ = dc.registries(dim, arch, mdr=dc.ALWAYS)
    q = rng.standard_normal((2, dim)).astype(F)
    for with_magnitude in (True, False):
        s = lib.encode_batch(rows, 0.5, with_magnitude)
        assert not s.host_arrays_present
        dot, mags = s.dot_dense(q), s.magnitudes()
        lib.set_min_device_rows(dc.NEVER)
        h = lib.encode_batch(rows, 0.5, with_magnitude)
        ha, sa = h.arrays(), s.arrays()
        assert s.nnz == h.nnz and all(np.array_equal(ha[k], sa[k]) for k in ("archetype_ids", "indptr", "positions", "has_cached", "sorted"))
        assert dc.same(ha["deltas"], sa["deltas"]) and dc.same(ha["cached_magnitudes"], sa["cached_magnitudes"])
        assert dc.same(dot, h.dot_dense(q)) and dc.same(mags, h.magnitudes())
        lib.set_min_device_rows(dc.ALWAYS)
    assert int(sa["indptr"][1024]) - int(sa["indptr"][1023]) >= 1 and sa["positions"][int(sa["indptr"][1024])] == 0
