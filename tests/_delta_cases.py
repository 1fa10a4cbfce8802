"""The cases of the delta-vector tests, shared by tests/test_delta_cpu.py (the library's host path, min_device_rows = NEVER) and
tests/test_gpu_delta.py (the device path, min_device_rows = 0): every check builds its inputs, runs the library and holds every
output to the twin tests/_delta_oracle.py bit for bit, a NaN compared as a NaN.  The shapes are the smallest at which each kernel can
go wrong; docs/delta.md §6 says which shape is there for which path."""
import numpy as np

from tests import _delta_oracle as do

F = np.float32
NEVER, ALWAYS = 2 ** 64 - 1, 0
FIND_DIMS = (1, 7, 63, 64, 65, 200)
FIND_KS = (7, 8, 9, 17)              # one below, at and one above the archetype tile of 8, and twice it plus one
FIND_NS = (1, 63, 65, 130)
ENCODE_DIMS = (63, 64, 65, 129)
THRESHOLDS = (0.0, -1.0, float("inf"), float("nan"), 1e-3)


def bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


def same(got, want):
    got, want = np.asarray(got, dtype=F), np.asarray(want, dtype=F)
    return got.shape == want.shape and bool(((bits(got) == bits(want)) | (np.isnan(got) & np.isnan(want))).all())


def registries(dim, archetypes, max_archetypes=None, mdr=NEVER):
    """the library's registry and the twin's, holding the same archetypes"""
    from neumann_amd import ArchetypeRegistry
    archetypes = np.asarray(archetypes, dtype=F).reshape(-1, dim)
    cap = len(archetypes) if max_archetypes is None else max_archetypes
    lib, twin = ArchetypeRegistry(dim, cap, min_device_rows=mdr), do.ArchetypeRegistry(cap)
    if len(archetypes):
        assert lib.register_batch(archetypes) == [twin.register(a) for a in archetypes]
    return lib, twin


def lib_set(lib, deltas):
    from neumann_amd import DeltaSet
    p = do.pack(deltas)
    return DeltaSet.from_parts(lib, p["archetype_ids"], p["indptr"], p["positions"], p["deltas"], p["cached_magnitudes"], p["has_cached"])


def assert_set_equals(s, deltas):
    a, p = s.arrays(), do.pack(deltas)
    assert len(s) == len(deltas) and s.nnz == int(p["indptr"][-1])
    assert np.array_equal(a["archetype_ids"], p["archetype_ids"]) and np.array_equal(a["indptr"], p["indptr"])
    assert np.array_equal(a["positions"], p["positions"]) and same(a["deltas"], p["deltas"])
    assert np.array_equal(a["has_cached"], p["has_cached"])
    assert same(a["cached_magnitudes"][p["has_cached"]], p["cached_magnitudes"][p["has_cached"]])
    assert same(s.compression_ratio(), [d.compression_ratio() for d in deltas])
    assert s.memory_bytes().tolist() == [d.memory_bytes() for d in deltas]


# ---- find_best ----------------------------------------------------------------------------------------------------------------

def find_inputs(dim, K, N, seed=0):
    rng = np.random.default_rng(seed + dim * 1000 + K * 10 + N)
    arch = rng.standard_normal((K, dim)).astype(F)
    if K > 1:
        arch[K - 1] = arch[0]                      # a duplicate across every tile border: the lower id wins
    if K > 4:
        arch[3] = 0.0                              # a zero archetype: its sim is 0.0
    rows = rng.standard_normal((N, dim)).astype(F)
    for i in range(0, N, 5):                       # rows near an archetype, so that the duplicate is the best of some
        rows[i] = arch[(i // 5) % K] * F(1.5) + F(0.01) * rows[i]
    if N > 2:
        rows[1] = 0.0                              # a zero row: (0, 0.0)
    if N > 6:
        rows[2, 0] = np.inf                        # query_mag is inf: every sim of a non-zero archetype is NaN
        rows[3, dim // 2] = np.nan
        rows[4] = -np.abs(arch[K - 1]) - 1         # a row that may have only negative sims except for the zero archetype
    return arch, rows


def check_find_best(mdr, dim, K, N):
    arch, rows = find_inputs(dim, K, N)
    lib, twin = registries(dim, arch, mdr=mdr)
    ids, sims = lib.find_best_batch(rows)
    want_ids, want_sims = twin.find_best_many(rows)
    assert np.array_equal(ids, want_ids), (ids, want_ids)
    assert same(sims, want_sims)
    assert same([lib.magnitude_sq(i) for i in range(K)], twin.magnitude_sq_)
    one = lib.find_best_archetype(rows[0])
    assert one[0] == want_ids[0] and same(one[1], want_sims[0])


def check_find_best_specials(mdr):
    """by hand: the zero archetype beats archetypes of only negative similarity with 0.0; equal sims: the first; all NaN: (0, -inf)"""
    dim = 9
    arch = np.zeros((10, dim), dtype=F)
    arch[:, 0] = -1.0
    arch[:, 1] = np.arange(10)
    arch[8] = 0.0                                  # the zero archetype sits in the second tile
    lib, twin = registries(dim, arch, mdr=mdr)
    rows = np.zeros((4, dim), dtype=F)
    rows[0, 0] = 1.0                               # every other sim is negative
    rows[1, 0] = -2.0                              # archetype 0 is the best, alone
    rows[2, 0] = np.inf
    rows[3, 5] = 1.0                               # orthogonal to all: every sim is 0.0 (or -0.0): the first wins
    ids, sims = lib.find_best_batch(rows)
    w_ids, w_sims = twin.find_best_many(rows)
    assert np.array_equal(ids, w_ids) and same(sims, w_sims)
    assert ids[0] == 8 and bits(sims[0]) == 0
    assert ids[1] == 0 and sims[1] == 1.0
    assert ids[2] == 8 and bits(sims[2]) == 0      # the zero archetype's 0.0 is the only sim that is not NaN
    # without the zero archetype every sim of the inf row is NaN: (0, -inf)
    lib2, twin2 = registries(dim, arch[:8], mdr=mdr)
    ids, sims = lib2.find_best_batch(rows)
    w_ids, w_sims = twin2.find_best_many(rows)
    assert np.array_equal(ids, w_ids) and same(sims, w_sims)
    assert ids[2] == 0 and sims[2] == -np.inf
    # duplicates: archetypes 1 and 9 of a registry of 10 are equal, as are 0 and 8
    arch3 = np.random.default_rng(3).standard_normal((10, dim)).astype(F)
    arch3[9], arch3[8] = arch3[1], arch3[0]
    lib3, twin3 = registries(dim, arch3, mdr=mdr)
    ids, _ = lib3.find_best_batch(arch3)
    assert ids.tolist() == [0, 1, 2, 3, 4, 5, 6, 7, 0, 1] and np.array_equal(ids, twin3.find_best_many(arch3)[0])


def check_empty_registry(mdr):
    lib, twin = registries(5, np.zeros((0, 5)), max_archetypes=4, mdr=mdr)
    rows = np.ones((3, 5), dtype=F)
    assert lib.find_best_batch(rows)[0].tolist() == [-1, -1, -1] and twin.find_best_many(rows) is None
    assert lib.find_best_archetype(rows[0]) is None and lib.encode(rows[0], 0.1) is None
    assert len(lib.encode_batch(rows, 0.1)) == 0 and twin.encode_batch(rows, 0.1) == []
    st = lib.analyze_coverage(rows, 0.1)
    assert (st.avg_similarity, st.avg_compression_ratio, st.avg_delta_nnz, st.archetype_usage) == (0.0, 0.0, 0.0, [])
    assert lib.get(0) is None and lib.magnitude_sq(0) is None and len(lib) == 0


# ---- encode -------------------------------------------------------------------------------------------------------------------

def encode_inputs(dim, n=300, seed=1):
    """rows that differ from an archetype in 0, 1, 63, 64, 65 and dim positions by 0.5, elsewhere by noise below 1e-3 or not at all;
    more rows than one block of the offset scan, so that the running total crosses its border"""
    rng = np.random.default_rng(seed + dim)
    arch = (rng.standard_normal((3, dim)) * 2).astype(F)
    rows = np.empty((n, dim), dtype=F)
    counts = [c for c in (0, 1, 63, 64, 65, dim) if c <= dim]
    for i in range(n):
        r = arch[i % 3].copy()
        c = counts[i % len(counts)]
        where = rng.permutation(dim)[:c]
        r[where] += F(0.5) * rng.choice([-1, 1], size=c).astype(F)
        if i % 7 == 1:
            noise = np.setdiff1d(np.arange(dim), where)[::2]
            r[noise] += (rng.standard_normal(noise.size) * 1e-4).astype(F)
        rows[i] = r
    rows[0] = arch[0]                              # a row equal to its archetype
    rows[7, dim - 1] = np.nan                      # a NaN and an inf delta in one row
    rows[7, 0] = np.inf
    return arch, rows


def check_encode(mdr, dim, threshold, with_magnitude):
    arch, rows = encode_inputs(dim)
    lib, twin = registries(dim, arch, mdr=mdr)
    s = lib.encode_batch(rows, threshold, with_magnitude)
    want = [d for d, _ in twin.encode_batch(rows, threshold, with_magnitude)]
    assert_set_equals(s, want)
    assert s.arrays()["sorted"].all()
    nnz = s.row_nnz()
    if threshold == 0.0:
        assert nnz[0] == 0 and {0, 1, dim}.issubset(set(nnz.tolist()))
    if threshold < 0:
        assert (np.delete(nnz, 7) == dim).all() and nnz[7] == dim - 1         # zero deltas are kept, the NaN is not
    if threshold != threshold or threshold == float("inf"):
        assert s.nnz == 0
    assert same(s.to_dense(), do.decode_all(twin, want))
    one = lib.encode(rows[5], threshold, with_magnitude)
    assert_set_equals(one, [twin.encode(rows[5], threshold, with_magnitude)])


def check_encode_wide(mdr):
    """one row at the largest dimension whose last position is kept; one dimension more is DimensionExceeded"""
    from neumann_amd import DeltaVectorError
    dim = do.MAX_DIMENSION
    arch = np.zeros((2, dim), dtype=F)
    arch[0, ::7], arch[1, ::5] = 1.0, -1.0
    row = arch[0].copy()
    row[dim - 1] += 3.0
    row[1000] -= 2.0
    lib, twin = registries(dim, arch, mdr=mdr)
    s = lib.encode_batch(row[None, :], 0.5, True)
    want = [twin.encode(row, 0.5, True)]
    assert_set_equals(s, want)
    assert s.positions.tolist() == [1000, dim - 1]
    lib2, _ = registries(dim + 1, np.zeros((1, dim + 1)), mdr=mdr)
    for call in (lambda: lib2.encode_batch(np.zeros((1, dim + 1)), 0.5), lambda: lib2.analyze_coverage(np.zeros((1, dim + 1)), 0.5)):
        try:
            call()
        except DeltaVectorError as e:
            assert str(e) == do.dimension_exceeded(dim + 1) == "dimension 65536 exceeds maximum 65535 (u16::MAX)"
        else:
            raise AssertionError("a dimension of 65536 was not refused")
    # on an empty registry `encode` is None before any DeltaVector is built: an empty set at any dimension, and the default stats
    lib0, twin0 = registries(dim + 1, np.zeros((0, dim + 1)), max_archetypes=1, mdr=mdr)
    assert len(lib0.encode_batch(np.zeros((2, dim + 1)), 0.5)) == 0 and twin0.encode_batch(np.zeros((2, dim + 1)), 0.5) == []
    assert len(lib2.encode_batch(np.zeros((0, dim + 1)), 0.5)) == 0
    assert lib0.analyze_coverage(np.zeros((2, dim + 1)), 0.5).archetype_usage == []
    ids, sims = lib2.find_best_batch(np.ones((1, dim + 1)))                     # find_best_archetype itself has no such limit
    assert ids.tolist() == [0] and bits(sims[0]) == 0


def check_coverage(mdr):
    arch, rows = encode_inputs(65, n=70)
    lib, twin = registries(65, arch, mdr=mdr)
    for threshold in (1e-3, 0.0):
        got, want = lib.analyze_coverage(rows[8:], threshold), twin.analyze_coverage(rows[8:], threshold)
        assert got.archetype_usage == want.archetype_usage
        assert same([got.avg_similarity, got.avg_compression_ratio, got.avg_delta_nnz],
                    [want.avg_similarity, want.avg_compression_ratio, want.avg_delta_nnz])
    got, want = lib.analyze_coverage(rows, 1e-3), twin.analyze_coverage(rows, 1e-3)      # with the NaN row: (0, -inf) joins the sum
    assert same(got.avg_similarity, want.avg_similarity) and want.avg_similarity == -np.inf
    assert got.archetype_usage == want.archetype_usage and same(got.avg_delta_nnz, want.avg_delta_nnz)


# ---- scoring ------------------------------------------------------------------------------------------------------------------

def score_inputs(dim=70, n=130, seed=2):
    """130 rows over 4 archetypes (one of them zero): slice 0 holds rows of 0 and of 65 entries; position 9 is stored by the rows
    3 mod 4 only, so a query with inf or NaN there must leave their slice neighbours finite"""
    rng = np.random.default_rng(seed)
    arch = rng.standard_normal((4, dim)).astype(F)
    arch[2] = 0.0
    twin = do.ArchetypeRegistry(4)
    for a in arch:
        twin.register(a)
    deltas = []
    for i in range(n):
        if i % 4 == 3:
            pos = np.sort(np.concatenate([[9], rng.permutation(np.setdiff1d(np.arange(dim), [9]))[:i % 7]]))
        elif i == 5:
            pos = np.arange(65)                    # 65 entries beside ...
            pos = pos[pos != 9]
            pos = np.concatenate([pos, [66]])
        elif i in (4, 6, 64, 129):
            pos = np.zeros(0, dtype=np.int64)      # ... rows of none
        else:
            pos = np.sort(rng.permutation(np.setdiff1d(np.arange(dim), [9]))[:rng.integers(0, 12)])
        cached = None if i % 3 or i in (4, 6) else F(abs(rng.standard_normal()) + 0.5)
        deltas.append(do.DeltaVector(i % 4 if i not in (4, 6) else 2, dim, pos, rng.standard_normal(len(pos)).astype(F), cached))
    return arch, twin, deltas


def score_queries(dim, nq, seed=5):
    rng = np.random.default_rng(seed + nq)
    q = rng.standard_normal((nq, dim)).astype(F)
    q[0] = -np.abs(q[0]) - F(0.1)                  # all negative: the zero archetype's dot is -0.0, and a row of no entries keeps it
    if nq > 1:
        q[1, 9] = np.inf
    if nq > 2:
        q[2, 9] = np.nan
        q[3] = 0.0                                 # a zero query: cosine is 0.0
    return q


def check_score(mdr, nq):
    arch, twin, deltas = score_inputs()
    lib, _ = registries(arch.shape[1], arch, mdr=mdr)
    s = lib_set(lib, deltas)
    q = score_queries(arch.shape[1], nq)
    want = do.dot_dense_all(twin, deltas, q)
    got = s.dot_dense(q)
    assert same(got, want)
    assert bits(want[0, 4]) == 0x80000000 and bits(got[0, 6]) == 0x80000000             # -0.0 + -0.0
    if nq > 2:
        # the archetype's own dot meets the inf as well: a row that does not store position 9 is +-inf, never the NaN that
        # inf - inf or 0 * inf of a neighbour's entry would make of it (the rows of the zero archetype are NaN: 0 * inf)
        plain = [i for i in range(len(deltas)) if i % 4 in (0, 1) and i not in (4, 6)]
        assert np.isinf(want[1, plain]).all() and np.isnan(want[2]).all()
    assert same(s.magnitudes(), do.magnitudes(twin, deltas))
    wcos = do.cosine_dense_all(twin, deltas, q)
    assert same(s.cosine_similarity_dense(q), wcos)
    assert bits(wcos[0, 4]) == 0 and bits(wcos[0, 6]) == 0                               # a zero row magnitude: 0.0
    if nq > 3:
        assert (bits(wcos[3]) == 0).all()
    assert same(lib.dot_delta_dense(s, q[0]), want[0])
    assert same(lib.decode(s), do.decode_all(twin, deltas))


def check_score_encoded(mdr):
    """the same through encode_batch, cached and not: the set the encoder leaves is the set from_parts makes"""
    arch, rows = encode_inputs(129, n=70)
    lib, twin = registries(129, arch, mdr=mdr)
    q = score_queries(129, 2)
    for with_magnitude in (False, True):
        s = lib.encode_batch(rows, 1e-3, with_magnitude)
        want = [d for d, _ in twin.encode_batch(rows, 1e-3, with_magnitude)]
        assert same(s.dot_dense(q), do.dot_dense_all(twin, want, q))
        assert same(s.cosine_similarity_dense(q), do.cosine_dense_all(twin, want, q))
        assert same(s.magnitudes(), do.magnitudes(twin, want))


def check_score_lds_limit(mdr, dim):
    """one row and two archetypes at a dimension just below / above the largest query kept in LDS"""
    rng = np.random.default_rng(dim)
    arch = rng.standard_normal((2, dim)).astype(F)
    lib, twin = registries(dim, arch, mdr=mdr)
    deltas = [do.DeltaVector(1, dim, [0, 17, dim - 1], [0.5, -2.0, 3.0])]
    q = rng.standard_normal((2, dim)).astype(F)
    s = lib_set(lib, deltas)
    assert same(s.dot_dense(q), do.dot_dense_all(twin, deltas, q))
    assert same(s.cosine_similarity_dense(q), do.cosine_dense_all(twin, deltas, q))


# ---- from_parts sets ----------------------------------------------------------------------------------------------------------

def parts_inputs(dim=40, seed=8):
    rng = np.random.default_rng(seed)
    arch = rng.standard_normal((3, dim)).astype(F)
    twin = do.ArchetypeRegistry(3)
    for a in arch:
        twin.register(a)
    big = F(2.0 ** 24)
    deltas = [
        do.DeltaVector(0, dim, [5, 3, 5, 5, 1], [big, 1.0, 1.0, -big, 2.0]),             # unsorted, repeated: the order shows in the bits
        do.DeltaVector(0, dim, [1, 3, 5, 7], [1.5, -2.5, 3.5, 4.5], F(2.0)),
        do.DeltaVector(0, dim, [1, 3, 5, 7], [0.5, 0.25, -3.0, 2.0]),                     # identical position lists
        do.DeltaVector(0, dim, [0, 2, 4, 6], [1.0, 2.0, 3.0, 4.0]),                       # disjoint
        do.DeltaVector(1, dim, [1, 3], [1.0, 1.0]),                                       # another archetype
        do.DeltaVector(1, dim, [], []),
        do.DeltaVector(2, dim, [7, 7], [1.0, 2.0]),
        do.DeltaVector(0, dim, [9, 8, 7, 3, 1], rng.standard_normal(5).astype(F)),        # descending: the merge loop skips as written
    ]
    for i in range(60):                            # past one 64-row slice
        m = int(rng.integers(0, 9))
        pos = rng.integers(0, dim, size=m) if i % 2 else np.sort(rng.permutation(dim)[:m])
        deltas.append(do.DeltaVector(int(rng.integers(0, 3)), dim, pos, rng.standard_normal(m).astype(F)))
    return arch, twin, deltas


def check_parts(mdr):
    arch, twin, deltas = parts_inputs()
    dim = arch.shape[1]
    lib, _ = registries(dim, arch, mdr=mdr)
    s = lib_set(lib, deltas)
    assert_set_equals(s, deltas)
    assert s.arrays()["sorted"][:8].tolist() == [False, True, True, True, True, True, False, False]
    dense = do.decode_all(twin, deltas)
    assert same(s.to_dense(), dense)
    assert dense[0, 5] != F(arch[0, 5] + F(1.0))                   # (a + 2^24 + 1 - 2^24 in that order is not a + 1)
    assert same(s.magnitudes(), do.magnitudes(twin, deltas))
    q = np.random.default_rng(4).standard_normal((2, dim)).astype(F)
    assert same(s.dot_dense(q), do.dot_dense_all(twin, deltas, q))
    assert same(s.cosine_similarity_dense(q), do.cosine_dense_all(twin, deltas, q))
    n = len(deltas)
    pairs = [(0, 1), (1, 2), (2, 1), (1, 3), (0, 0), (7, 1), (1, 7), (0, 7), (4, 5), (1, 4), (6, 6), (5, 5)]
    pairs += [(i, (i * 7 + 3) % n) for i in range(n)]
    got, ok = lib.dot_deltas_same_archetype(s, s, pairs)
    want, wok = do.pairs_all(twin, deltas, deltas, pairs)
    assert np.array_equal(ok, wok) and same(got[ok], want[wok])
    assert not ok[9] and ok[:9].all() and 3 < ok.sum() < len(pairs)
    t = lib_set(lib, deltas[::-1])                                  # two different sets of one registry
    got, ok = lib.dot_deltas_same_archetype(s, t)
    want, wok = do.pairs_all(twin, deltas, deltas[::-1], [(i, i) for i in range(n)])
    assert np.array_equal(ok, wok) and same(got[ok], want[wok])


def check_refusals(mdr):
    from neumann_amd import ArchetypeRegistry, DeltaSet, DeltaVectorError
    lib, _ = registries(8, np.ones((2, 8)), mdr=mdr)

    def refused(text, *args):
        try:
            DeltaSet.from_parts(lib, *args)
        except DeltaVectorError as e:
            assert text in str(e), str(e)
        else:
            raise AssertionError(f"not refused: {text}")
    refused("row 1: archetype id 2 is not registered (the registry holds 2)", [0, 2], [0, 1, 2], [1, 2], [1.0, 2.0])
    refused("row 1: indptr does not ascend", [0, 1], [0, 2, 1], [1, 2], [1.0, 2.0])
    refused("indptr[0] must be 0", [0], [1, 2], [1, 2], [1.0, 2.0])
    refused("row 0: position 8 is not below the dimension 8", [0], [0, 2], [1, 8], [1.0, 2.0])
    refused("position 70000 is not below the dimension 8", [0], [0, 1], [70000], [1.0])
    refused("indptr must hold 2 offsets", [0], [0, 1, 2], [1, 2], [1.0, 2.0])
    refused("must both hold", [0], [0, 3], [1, 2], [1.0, 2.0])
    other, _ = registries(8, np.ones((2, 8)), mdr=mdr)
    a, b = DeltaSet.from_parts(lib, [0], [0, 1], [1], [1.0]), DeltaSet.from_parts(other, [0], [0, 1], [1], [1.0])
    for call, text in ((lambda: lib.dot_deltas_same_archetype(a, b), "another registry"),
                       (lambda: lib.dot_deltas_same_archetype(a, a, [(0, 1)]), "pair 0 names a row its set does not hold"),
                       (lambda: ArchetypeRegistry(0, 4), "a dimension of at least 1"),
                       (lambda: lib.find_best_batch(np.ones((2, 7))), "must be [n][8]")):
        try:
            call()
        except DeltaVectorError as e:
            assert text in str(e), str(e)
        else:
            raise AssertionError(f"not refused: {text}")
    # register returns None at max_archetypes, for every further row
    assert lib.register(np.ones(8)) is None and len(lib) == 2
    cap3, _ = registries(8, np.ones((2, 8)), max_archetypes=3, mdr=mdr)
    assert cap3.register_batch(np.ones((3, 8))) == [2, None, None]
