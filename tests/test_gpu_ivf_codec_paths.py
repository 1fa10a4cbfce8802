"""Every kernel path of the IVF-PQ / IVF-Binary storages (neumann_amd/csrc/nmn_ivf_codec.hip and the codec halves of
nmn_ivf.hip) against tests/_ivf_codec_oracle.py, bit for bit: the paths the small shapes of test_gpu_ivf_pq.py /
test_gpu_ivf_binary.py never take — a list scanned by more than one workgroup, the ADC table and the encoder's codebook at and
beyond the LDS budget, several 16-byte code reads per row, the residual kernel's grid-stride trip, an `add` of more rows than
one quantize launch and one staging pass hold, and the word / thread-count edges of the binary quantizer.

Every case gives the GPU index and the oracle the same trained state (centroids +-4 on every coordinate, unit-variance rows
around them, so list sizes can be arranged exactly), and checks `add`'s clusters, `codes()`, `cluster_sizes()` and, for BOTH
`search` and `search_device`, ids, distance bits, counts and padding against the oracle itself.  The oracle side goes through
the batch helpers (`add_rows` ...), which tests/test_ivf_codec_cpu.py holds to their scalar originals.  Each case asserts the
inequality that puts it on its path; the thresholds below are compared with the kernels' own definitions in
tests/test_ivf_codec_cpu.py::test_codec_path_thresholds_match_the_kernels."""
import numpy as np
import pytest

from tests import _ivf_codec_oracle as co

pytestmark = pytest.mark.gpu
F = np.float32
NONE = np.uint64(0xFFFFFFFFFFFFFFFF)
FAST = dict(max_iterations=2, convergence_threshold=1.0, seed=42, init_method="random")  # ivf.rs:589-596
METHODS = ["sign", "mean", "median"]

# ---- the thresholds the cases rely on (nmn_ivf_codec.hip unless said otherwise) ----------------------------------------
SCAN_ROWS_PER_BLOCK = 1024        # `constexpr uint32_t kCodecRowsPerBlock = 1024;` rows of a list per scan workgroup
LDS_BUDGET = 64 * 1024            # `constexpr size_t kLdsBudget = 64 * 1024;` `lds <= kLdsBudget` takes the LDS variant
CODE_VECTOR_BYTES = 16            # `(M & 15u) == 0` in pq_scan_kernel: codes read as uint4, M / 16 trips per row
BQ_ROWS_PER_LAUNCH = 65535        # `for (uint64_t r0 = 0; r0 < n; r0 += 65535)` in launch_bq_quantize
ADD_STAGE_ROWS = 65536            # `kStage = std::min<uint64_t>(n, 65536)` in codec_add (nmn_ivf.hip)
RESIDUAL_MAX_BLOCKS = 8192        # `std::min<uint64_t>((n * dim + 255) / 256, 8192)` in launch_pq_residual
RESIDUAL_BLOCK = 256              # ... blocks of 256 threads, one element per thread and trip
ENCODE_ROWS_PER_GRID = 1024 * 256  # `std::min<uint64_t>((n + 255) / 256, 1024)` blocks of 256 rows in launch_pq_encode


def table_bytes(M, K):
    """dynamic LDS pq_scan_kernel<true> asks for: `(size_t)M * Kt * 4`, Kt = min(K, 256)"""
    return M * min(K, 256) * 4


def codebook_bytes(M, K, dim):
    """dynamic LDS pq_encode_kernel<true> asks for: `(size_t)K * subdim * 4`"""
    return K * (dim // M) * 4


# ---- data -----------------------------------------------------------------------------------------------------------
def centroids(C, dim):
    """C <= 4 well separated centroids, +-4 on every coordinate: list c flips the even coordinates when c & 1, the odd ones
    when c & 2 (dim 1: only lists 0 and 1 differ)"""
    assert C <= 4 and (dim >= 2 or C <= 2)
    j = np.arange(dim)
    return np.stack([np.where((c >> (j % 2)) & 1, F(-4.0), F(4.0)) for c in range(C)]).astype(F)


def rows_in_lists(sizes, dim, seed):
    """unit-variance rows around centroids(len(sizes), dim), sizes[c] of them around centroid c, ids shuffled over the lists"""
    rng = np.random.default_rng(seed)
    labels = np.repeat(np.arange(len(sizes)), sizes)
    rng.shuffle(labels)
    cents = centroids(len(sizes), dim)
    return cents, (cents[labels] + rng.standard_normal((len(labels), dim))).astype(F), labels


def queries(cents, V, seed, nq=5):
    """Q[0] is a stored row; the others sit around the centroids in turn, so nprobe = 1 probes every list"""
    rng = np.random.default_rng(seed)
    Q = (cents[np.arange(nq) % len(cents)] + rng.standard_normal((nq, cents.shape[1]))).astype(F)
    Q[0] = V[len(V) // 3]
    return Q


def random_codebook(M, K, dim, seed):
    sub = dim // M
    cb = np.random.default_rng(seed).standard_normal((M, K, sub)).astype(F)
    return co.PQCodebook(sub, M, K, cb, dim)


def make_pq(cents, M, K, capacity, seed, nprobe=None):
    from neumann_amd.ivf import GpuIvfPQ
    book = random_codebook(M, K, cents.shape[1], seed)
    orc = co.IVFCoded(len(cents), "pq", pq_config=co.PQConfig(M, K), nprobe=nprobe)
    orc.set_trained(cents, book)
    gpu = GpuIvfPQ(cents, book.centroids, capacity_rows=capacity, num_subspaces=M, nprobe=orc.nprobe)
    assert gpu.num_codewords == K
    return orc, gpu


def make_binary(cents, method, capacity, nprobe=None):
    from neumann_amd.ivf import GpuIvfBinary
    orc = co.IVFCoded(len(cents), "binary", threshold=method, nprobe=nprobe)
    orc.set_trained(cents)
    return orc, GpuIvfBinary(cents, capacity_rows=capacity, threshold=method, nprobe=orc.nprobe)


# ---- checks ---------------------------------------------------------------------------------------------------------
def assert_rows_equal(got, want, what):
    """equal arrays, or the first differing row by name (the rows around a launch or stage boundary are the telling ones)"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, f"{what}: shape {got.shape}, want {want.shape}"
    if not np.array_equal(got, want):
        bad = np.flatnonzero((got != want).reshape(len(got), -1).any(axis=1))
        r = int(bad[0])
        raise AssertionError(f"{what}: {len(bad)} of {len(got)} rows differ, the first at row {r}: got {got[r]!r}, want {want[r]!r}; "
                             f"differing rows {bad[:8].tolist()} ... {bad[-4:].tolist()}")


def add_and_check(orc, gpu, V):
    """one `add` of all of V on the GPU, add_rows in the oracle: clusters, codes, list sizes"""
    got = gpu.add(V)
    want = orc.add_rows(V)
    assert_rows_equal(got, np.asarray(want, np.uint32), "clusters returned by add")
    assert len(gpu) == len(orc.codes)
    assert_rows_equal(gpu.codes(), np.stack(orc.codes), "codes()")
    assert gpu.cluster_sizes().tolist() == orc.cluster_sizes()
    assert gpu.list_major_rows == len(orc.codes)


def dev(Q):
    import torch
    return torch.from_numpy(np.ascontiguousarray(Q, dtype=F)).cuda()


def host(res):
    ids, dist, counts = res
    return ids.cpu().numpy().view(np.uint64), dist.cpu().numpy(), counts.cpu().numpy().astype(np.uint32)


def check_searches(orc, gpu, Q, ks, nprobes, nqs=(None,)):
    """`search` and `search_device`, each against the oracle: the oracle answers every (query, nprobe) once at the largest k
    — its stable sort cut at k is a prefix of the one cut at any larger k — and each call is compared with that prefix"""
    Q = np.atleast_2d(np.asarray(Q, F))
    nqs = [len(Q) if n is None else n for n in nqs]
    kmax = max(ks)
    for nprobe in nprobes:
        ref = []
        for q in Q[:max(nqs)]:
            eids, ed = orc.search(q, kmax, nprobe)
            ref.append((np.asarray(eids, np.uint64), np.asarray(ed, F)))
        for nq in nqs:
            Qd = dev(Q[:nq])
            for k in ks:
                answers = (("search", gpu.search(Q[:nq], k, nprobe)), ("search_device", host(gpu.search_device(Qd, k, nprobe))))
                for name, (ids, dist, counts) in answers:
                    at = f"{name}(nq={nq}, k={k}, nprobe={nprobe})"
                    assert ids.shape == (nq, k) and dist.shape == (nq, k) and counts.shape == (nq,), at
                    for i in range(nq):
                        eids, ed = ref[i][0][:k], ref[i][1][:k]
                        n = len(eids)
                        assert counts[i] == n, f"{at} query {i}: count {counts[i]}, want {n}"
                        assert_rows_equal(ids[i, :n], eids, f"{at} query {i}: ids")
                        assert_rows_equal(dist[i, :n].view(np.uint32), ed.view(np.uint32), f"{at} query {i}: distance bits")
                        assert np.all(ids[i, n:] == NONE) and np.all(np.isposinf(dist[i, n:])), f"{at} query {i}: padding"
    return ref


# ---- a. lists longer than one scan workgroup ---------------------------------------------------------------------------
LONG_SIZES = [SCAN_ROWS_PER_BLOCK, SCAN_ROWS_PER_BLOCK + 1, 2151]  # 1 workgroup exactly, 1 + a 1-row tail, 3 workgroups
LONG_STORAGES = [("pq", 4, 16), ("pq", 16, 16), ("binary", "sign", 16), ("binary", "mean", 16), ("binary", "median", 16),
                 ("binary", "sign", 130)]


@pytest.mark.parametrize("storage", LONG_STORAGES, ids=lambda s: "-".join(map(str, s)))
def test_lists_longer_than_one_scan_workgroup(storage):
    """blockIdx.y > 0 of pq_scan_kernel / bq_scan_kernel: lists of exactly 1024, 1025 and 2151 rows; K = 16 (and Binary's
    dim + 1 values) give runs of equal distances across the 1024-row seams, whose order the stable sort fixes"""
    kind, arg, dim = storage
    assert LONG_SIZES[0] == SCAN_ROWS_PER_BLOCK and LONG_SIZES[1] == SCAN_ROWS_PER_BLOCK + 1
    assert LONG_SIZES[2] >= 2 * SCAN_ROWS_PER_BLOCK + 1
    cents, V, labels = rows_in_lists(LONG_SIZES, dim, seed=100)
    if kind == "pq":
        assert (arg % CODE_VECTOR_BYTES == 0) == (arg == 16) and table_bytes(arg, 16) <= LDS_BUDGET
        orc, gpu = make_pq(cents, arg, 16, len(V), seed=101)
    else:
        assert (dim + 63) // 64 == (3 if dim == 130 else 1)
        orc, gpu = make_binary(cents, arg, len(V))
    with gpu:
        clusters = gpu.add(V)
        assert gpu.cluster_sizes().tolist() == LONG_SIZES  # the premise of this case, before anything else
        assert_rows_equal(clusters, np.asarray(orc.add_rows(V), np.uint32), "clusters returned by add")
        assert clusters.tolist() == labels.tolist()
        assert_rows_equal(gpu.codes(), np.stack(orc.codes), "codes()")
        assert orc.cluster_sizes() == LONG_SIZES
        Q = queries(cents, V, seed=102)
        ref = check_searches(orc, gpu, Q, ks=(1, 100, 1024, 1025, 4096, 5000), nprobes=(1, len(cents)), nqs=(1, 5))
        # (ref: the oracle's answers at nprobe = all, k = 5000) every row is a candidate, the stored row among them ...
        assert all(len(ids) == len(V) for ids, _ in ref) and len(V) // 3 in ref[0][0]
        if kind == "binary":
            assert ref[0][1][0] == 0.0
        if arg != 16:  # ... and distances repeat (M = 16 codes over 16 one-dimensional subspaces hardly ever do)
            assert all(len(set(d.tolist())) < len(V) - 100 for _, d in ref)


# ---- b. the ADC table at and beyond LDS ---------------------------------------------------------------------------------
@pytest.mark.parametrize("M,K,dim,lds,vec", [(32, 64, 64, True, True), (64, 256, 64, True, True), (80, 256, 80, False, True),
                                             (72, 256, 144, False, False)])
def test_adc_table_at_and_beyond_lds(M, K, dim, lds, vec):
    """pq_scan_kernel<true> with 2 and 4 sixteen-byte trips, the latter at exactly the LDS budget; pq_scan_kernel<false>
    with 16-byte and with byte-wise code reads"""
    assert (table_bytes(M, K) <= LDS_BUDGET) == lds and (M % CODE_VECTOR_BYTES == 0) == vec
    if (M, K) == (64, 256):
        assert table_bytes(M, K) == LDS_BUDGET
    if vec:
        assert M // CODE_VECTOR_BYTES >= 2
    cents, V, _ = rows_in_lists([140, 160], dim, seed=110)
    orc, gpu = make_pq(cents, M, K, len(V), seed=111)
    with gpu:
        add_and_check(orc, gpu, V)
        check_searches(orc, gpu, queries(cents, V, seed=112, nq=3), ks=(10, 300), nprobes=(2,))


# ---- c. the encoder's codebook at and beyond LDS --------------------------------------------------------------------------
@pytest.mark.parametrize("M,K,dim,lds", [(1, 256, 64, True), (1, 256, 128, False), (8, 256, 768, False), (1, 300, 64, False)])
def test_encoder_codebook_at_and_beyond_lds(M, K, dim, lds):
    """pq_encode_kernel<true> at exactly the LDS budget and pq_encode_kernel<false> beyond it — (8, 256, 768) is the
    reference's default PQConfig at 768 dimensions; K = 300 also wraps the codes"""
    assert (codebook_bytes(M, K, dim) <= LDS_BUDGET) == lds
    if (M, K, dim) == (1, 256, 64):
        assert codebook_bytes(M, K, dim) == LDS_BUDGET
    cents, V, _ = rows_in_lists([140, 160], dim, seed=120)
    orc, gpu = make_pq(cents, M, K, len(V), seed=121)
    with gpu:
        add_and_check(orc, gpu, V)
        if K > 256:
            cb, R = orc.codebook, (V - cents[np.asarray(orc.assign)]).astype(F)
            first = np.argmin(np.stack([co.sq_dist_rows(cb.centroids[0], r) for r in R[:, :dim // M]]), axis=1)
            assert (first >= 256).any()  # some codes did wrap
        check_searches(orc, gpu, queries(cents, V, seed=122, nq=3), ks=(10, 300), nprobes=(2,))


# ---- d. the default configuration through build ---------------------------------------------------------------------------
def test_default_pq_config_at_768_through_build():
    """GpuIvfPQ.build with PQConfig::default (M = 8, K = 256) at 768 dimensions: 96 KiB of codebook per subspace, so the
    build encodes with pq_encode_kernel<false>; centroids and codebook bit-equal to the oracle's train"""
    from neumann_amd.ivf import GpuIvfPQ
    M, K, dim, C = 8, 256, 768, 4
    assert codebook_bytes(M, K, dim) > LDS_BUDGET and table_bytes(M, K) <= LDS_BUDGET
    _, V, _ = rows_in_lists([100, 100, 100, 100], dim, seed=130)
    km = co.KMeansConfig(**FAST)
    orc = co.IVFCoded(C, "pq", pq_config=co.PQConfig(M, K, km), nprobe=2, kmeans=km)
    orc.train(V)
    orc.add_rows(V)
    with GpuIvfPQ.build(V, C, num_subspaces=M, num_centroids=K, pq_kmeans=FAST, nprobe=2, **FAST) as gpu:
        assert gpu.num_codewords == K and len(gpu) == len(V)
        assert_rows_equal(gpu.centroids().view(np.uint32), orc.centroids.view(np.uint32), "centroids")
        assert_rows_equal(gpu.codebook().view(np.uint32).reshape(M * K, -1), orc.codebook.centroids.view(np.uint32).reshape(M * K, -1),
                          "codebook")
        assert_rows_equal(gpu.codes(), np.stack(orc.codes), "codes()")
        assert gpu.cluster_sizes().tolist() == orc.cluster_sizes()
        check_searches(orc, gpu, np.concatenate([V[7:8], V[200:202] + F(0.25)]), ks=(20,), nprobes=(2,))


# ---- e. the residual kernel's grid-stride trip ----------------------------------------------------------------------------
def test_residual_grid_stride_trip():
    """one add of 8200 x 256: 2 099 200 elements against the 8192 x 256 threads of pq_residual_kernel's capped grid, so the
    first 2048 threads take a second trip"""
    n, dim, M, K = 8200, 256, 8, 16
    assert n * dim > RESIDUAL_MAX_BLOCKS * RESIDUAL_BLOCK and n <= ENCODE_ROWS_PER_GRID and n <= ADD_STAGE_ROWS
    cents, V, _ = rows_in_lists([4000, 4200], dim, seed=140)
    orc, gpu = make_pq(cents, M, K, n, seed=141)
    with gpu:
        add_and_check(orc, gpu, V)
        check_searches(orc, gpu, queries(cents, V, seed=142, nq=2), ks=(10,), nprobes=(2,))


# ---- f. an add beyond one quantize launch and one stage ---------------------------------------------------------------
@pytest.mark.parametrize("storage", [("binary", "sign"), ("binary", "mean"), ("binary", "median"), ("pq", 2)],
                         ids=lambda s: "-".join(map(str, s)))
def test_add_beyond_one_launch_and_one_stage(storage):
    """one add of 65 536 + 300 rows: launch_bq_quantize's second launch starts at row 65 535, codec_add's second stage at
    row 65 536 (staging index reused from its row 0); then both selections over 65 836 candidates, and a re-layout"""
    kind, arg = storage
    n, dim = ADD_STAGE_ROWS + 300, 8
    assert n > ADD_STAGE_ROWS > BQ_ROWS_PER_LAUNCH and n <= ENCODE_ROWS_PER_GRID
    cents, V, _ = rows_in_lists([n // 2, n - n // 2], dim, seed=150)
    more = rows_in_lists([4, 6], dim, seed=151)[1]
    if kind == "pq":
        orc, gpu = make_pq(cents, arg, 16, n + len(more), seed=152)
    else:
        orc, gpu = make_binary(cents, arg, n + len(more))
    with gpu:
        add_and_check(orc, gpu, V)
        assert min(orc.cluster_sizes()) > SCAN_ROWS_PER_BLOCK
        Q = queries(cents, V, seed=153, nq=2)
        Q[0] = V[ADD_STAGE_ROWS]  # the first row of the second stage
        check_searches(orc, gpu, Q, ks=(10, 5000), nprobes=(2,))
        add_and_check(orc, gpu, more)  # codes() again covers every earlier row
        check_searches(orc, gpu, Q[:1], ks=(5000,), nprobes=(2,))


# ---- g. the binary quantizer's word and thread-count edges ----------------------------------------------------------------
def ulp_run(start, count, back=0):
    """`count` consecutive floats, `back` of them below `start`"""
    return (np.asarray(start, F).view(np.uint32) - np.uint32(back) + np.arange(count, dtype=np.uint32)).view(F)


def binary_edge_rows(dim, seed):
    cents, V, _ = rows_in_lists([48, 48], dim, seed)
    rng = np.random.default_rng(seed + 1)
    mid = dim // 2
    V[3] = F(0.75)                                                   # all equal
    V[7] = np.where(rng.random(dim) < 0.5, F(0.0), F(-0.0))          # a zero row of both signs
    V[11] = -np.abs(V[11]) - F(0.5)                                  # all negative
    V[15] = rng.permutation(ulp_run(1.0, dim))                       # consecutive floats: keys differ in the low byte(s) only
    V[19] = rng.permutation(ulp_run(2.0, dim, back=mid))             # ... straddling a power of two
    V[23] = rng.permutation(-ulp_run(0.5, dim, back=mid))            # ... negative, where the key order reverses
    if dim >= 2:
        s = np.sort(V[27])
        s[mid - 1] = s[mid]                                          # the two middle ranks equal
        V[27] = rng.permutation(s)
        s = np.sort(V[31])
        s[mid - 1] = np.nextafter(s[mid], F(-np.inf), dtype=F)       # ... one ulp apart
        V[31] = rng.permutation(s)
        V[35] = np.repeat(V[35, :(dim + 1) // 2], 2)[:dim]           # every value twice
        V[39] = np.where(np.arange(dim) < mid, F(-1.5), F(2.5))      # two values only: the midpoint between them
    assert np.all(np.isfinite(V)) and np.all((V == 0) | (np.abs(V) >= np.finfo(F).tiny))  # finite and normal (or zero)
    return cents, V


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("dim", [1, 2, 63, 64, 65, 128, 129, 257, 1000])
def test_binary_word_and_thread_edges(dim, method):
    """bq_quantize_kernel where a word fills exactly, overflows by one bit, where dim passes the 256 threads of the
    workgroup (the radix select's and the word loop's strides) and where dim is no multiple of 64 beyond them"""
    cents, V = binary_edge_rows(dim, seed=160 + dim)
    orc, gpu = make_binary(cents, method, len(V))
    with gpu:
        add_and_check(orc, gpu, V)
        Q = np.concatenate([V[15:16], V[31:32], queries(cents, V, seed=161, nq=2)[1:]])
        check_searches(orc, gpu, Q, ks=(10, 200), nprobes=(2,))
