"""Delta vectors on the device (docs/delta.md): every kernel of nmn_delta.hip forced with min_device_rows = 0 and held to the twin
tests/_delta_oracle.py bit for bit on the cases of tests/_delta_cases.py; discover_archetypes against the twin's k-means; the
stream-ordered forms against the host-buffer forms; two threads on one set; and every answer unchanged by the calls before it."""
import threading

import numpy as np
import pytest

from oracle import ivf_oracle as io
from tests import _delta_cases as dc
from tests import _delta_oracle as do

pytestmark = pytest.mark.gpu
F = np.float32
DEV = dc.ALWAYS


@pytest.mark.parametrize("dim", dc.FIND_DIMS)
@pytest.mark.parametrize("K", dc.FIND_KS)
def test_find_best(dim, K):
    dc.check_find_best(DEV, dim, K, 130)


@pytest.mark.parametrize("N", dc.FIND_NS)
def test_find_best_rows(N):
    dc.check_find_best(DEV, 65, 9, N)


def test_find_best_specials_and_empty_registry():
    dc.check_find_best_specials(DEV)
    dc.check_empty_registry(DEV)


@pytest.mark.parametrize("threshold", dc.THRESHOLDS)
@pytest.mark.parametrize("dim", dc.ENCODE_DIMS)
def test_encode(dim, threshold):
    dc.check_encode(DEV, dim, threshold, dim % 2 == 1)
    if dim == 65:
        dc.check_encode(DEV, dim, threshold, False)


def test_encode_at_the_largest_dimension():
    dc.check_encode_wide(DEV)


def test_coverage():
    dc.check_coverage(DEV)


@pytest.mark.parametrize("nq", (1, 2, 5))
def test_scores(nq):
    dc.check_score(DEV, nq)


def test_scores_of_encoded_sets():
    dc.check_score_encoded(DEV)


@pytest.mark.parametrize("above", (0, 1))
def test_scores_at_the_lds_limit(above):
    from neumann_amd import delta
    dc.check_score_lds_limit(DEV, delta.limits()[1] + above)


def test_scores_of_more_queries_than_one_launch_takes():
    """65537 queries: the score kernels take them in blocks of 32768 (a grid's y is 16 bits wide); every block's offsets into the
    queries, the scratch and the output are held to the host path, and the blocks' borders to the twin"""
    rng = np.random.default_rng(11)
    arch = rng.standard_normal((2, 3)).astype(F)
    lib, twin = dc.registries(3, arch, mdr=DEV)
    deltas = [do.DeltaVector(0, 3, [1], [0.5]), do.DeltaVector(1, 3, [], []), do.DeltaVector(1, 3, [2, 0], [1.0, -2.0], F(1.5))]
    s = dc.lib_set(lib, deltas)
    q = rng.standard_normal((65537, 3)).astype(F)
    dot, cos = s.dot_dense(q), s.cosine_similarity_dense(q)
    lib.set_min_device_rows(dc.NEVER)
    assert dc.same(dot, s.dot_dense(q)) and dc.same(cos, s.cosine_similarity_dense(q))
    edge = [0, 32767, 32768, 65535, 65536]
    assert dc.same(dot[edge], do.dot_dense_all(twin, deltas, q[edge])) and dc.same(cos[edge], do.cosine_dense_all(twin, deltas, q[edge]))


def test_from_parts_sets_and_pairs():
    dc.check_parts(DEV)


def test_device_and_host_paths_agree_on_one_handle():
    """the same handle answers on either side of min_device_rows with the same bits"""
    arch, rows = dc.encode_inputs(65, n=70)
    lib, _ = dc.registries(65, arch, mdr=DEV)
    q = dc.score_queries(65, 2)
    dev = lib.encode_batch(rows, 1e-3, True)
    got = [lib.find_best_batch(rows)[1], dev.deltas, dev.dot_dense(q), dev.cosine_similarity_dense(q), dev.to_dense(), dev.magnitudes()]
    lib.set_min_device_rows(dc.NEVER)
    host = lib.encode_batch(rows, 1e-3, True)
    want = [lib.find_best_batch(rows)[1], host.deltas, dev.dot_dense(q), dev.cosine_similarity_dense(q), dev.to_dense(), dev.magnitudes()]
    assert all(dc.same(g, w) for g, w in zip(got, want))
    assert np.array_equal(dev.indptr, host.indptr) and np.array_equal(dev.positions, host.positions)


# ---- discover -------------------------------------------------------------------------------------------------------------------

def blobs(n=90, dim=12, seed=3):
    rng = np.random.default_rng(seed)
    centers = rng.standard_normal((4, dim)).astype(F) * 4
    return (centers[rng.integers(0, 4, size=n)] + rng.standard_normal((n, dim)).astype(F) * F(0.3)).astype(F)


@pytest.mark.parametrize("init", ("kmeans++", "random"))
def test_discover_equals_the_twin(init):
    from neumann_amd import ArchetypeRegistry
    rows = blobs()
    cfg = io.KMeansConfig(max_iterations=20, seed=7, init_method=init)
    lib, twin = ArchetypeRegistry(12, 6, min_device_rows=DEV), do.ArchetypeRegistry(6)
    kw = dict(max_iterations=20, seed=7, init_method=init)
    assert lib.discover_archetypes(rows, 4, **kw) == twin.discover_archetypes(rows, 4, cfg) == 4
    assert lib.discover_archetypes(rows[:50], 5, **kw) == twin.discover_archetypes(rows[:50], 5, cfg) == 2      # k > the room left: appends 2
    assert len(lib) == 6
    for i in range(6):
        assert dc.same(lib.get(i), twin.get(i)) and dc.same(lib.magnitude_sq(i), twin.magnitude_sq(i)), i
    assert lib.discover_archetypes(rows, 3, **kw) == twin.discover_archetypes(rows, 3, cfg) == 0                # a full registry
    assert lib.discover_archetypes(rows[:0], 3, **kw) == 0
    ids, sims = lib.find_best_batch(rows)
    w_ids, w_sims = twin.find_best_many(rows)
    assert np.array_equal(ids, w_ids) and dc.same(sims, w_sims)
    small, small_twin = ArchetypeRegistry(12, 16, min_device_rows=DEV), do.ArchetypeRegistry(16)                 # k > n
    assert small.discover_archetypes(rows[:3], 8, **kw) == small_twin.discover_archetypes(rows[:3], 8, cfg) == 3
    assert all(dc.same(small.get(i), small_twin.get(i)) for i in range(3))


# ---- stream-ordered forms ---------------------------------------------------------------------------------------------------------

def test_device_buffer_forms_equal_the_host_buffer_forms_on_a_side_stream():
    import torch
    from neumann_amd import DeltaVectorError
    arch, twin, deltas = dc.score_inputs()
    dim = arch.shape[1]
    lib, _ = dc.registries(dim, arch, mdr=DEV)
    s = dc.lib_set(lib, deltas)
    q = dc.score_queries(dim, 5)
    rows = dc.find_inputs(dim, 4, 130)[1]
    with pytest.raises(DeltaVectorError, match="not resident"):
        lib.find_best_device(torch.zeros((1, dim), dtype=torch.float32, device="cuda"))
    lib.to_device()
    with pytest.raises(DeltaVectorError, match="delta set is not resident"):
        s.dot_dense_device(torch.zeros((1, dim), dtype=torch.float32, device="cuda"))
    s.to_device()
    side = torch.cuda.Stream()
    tq, tr = torch.from_numpy(q).cuda(), torch.from_numpy(rows).cuda()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        ids, sims = lib.find_best_device(tr)
        dot = s.dot_dense_device(tq)
        cos = s.cosine_similarity_dense_device(tq)
    side.synchronize()
    # a raw stream handle and a scratch of the caller's, reused across the two calls
    scratch = torch.empty(s.scratch_floats(5), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    dot2 = s.dot_dense_device(tq, stream=side.cuda_stream, scratch=scratch)
    cos2 = s.cosine_similarity_dense_device(tq, stream=side.cuda_stream, scratch=scratch)
    dot3 = s.dot_dense_device(tq, stream=side.cuda_stream)
    side.synchronize()
    assert dc.same(dot2.cpu().numpy(), dot.cpu().numpy()) and dc.same(cos2.cpu().numpy(), cos.cpu().numpy())
    assert dc.same(dot3.cpu().numpy(), dot.cpu().numpy())
    w_ids, w_sims = lib.find_best_batch(rows)
    assert np.array_equal(ids.cpu().numpy(), w_ids) and dc.same(sims.cpu().numpy(), w_sims)
    assert dc.same(dot.cpu().numpy(), s.dot_dense(q)) and dc.same(cos.cpu().numpy(), s.cosine_similarity_dense(q))
    assert dc.same(dot.cpu().numpy(), do.dot_dense_all(twin, deltas, q))
    empty, _ = dc.registries(dim, np.zeros((0, dim)), max_archetypes=2, mdr=DEV)
    with pytest.raises(DeltaVectorError, match="registry is empty"):
        empty.to_device().find_best_device(tr)


# ---- concurrency and history ------------------------------------------------------------------------------------------------------

def test_two_threads_on_one_set_get_the_answers_of_one():
    arch, twin, deltas = dc.score_inputs()
    lib, _ = dc.registries(arch.shape[1], arch, mdr=DEV)
    s = dc.lib_set(lib, deltas)
    q = dc.score_queries(arch.shape[1], 5)
    rows = dc.find_inputs(arch.shape[1], 4, 130)[1]
    want = (do.dot_dense_all(twin, deltas, q), do.cosine_dense_all(twin, deltas, q), twin.find_best_many(rows)[1])
    results, errors = {}, []

    def work(name):
        try:
            for _ in range(3):
                results[name] = (s.dot_dense(q), s.cosine_similarity_dense(q), lib.find_best_batch(rows)[1], s.to_dense())
        except Exception as e:      # noqa: BLE001
            errors.append(e)
    threads = [threading.Thread(target=work, args=(i,)) for i in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    for r in results.values():
        assert all(dc.same(g, w) for g, w in zip(r[:3], want)) and dc.same(r[3], do.decode_all(twin, deltas))


def test_no_answer_depends_on_the_calls_before_it():
    arch, twin, deltas = dc.parts_inputs()
    dim = arch.shape[1]
    lib, _ = dc.registries(dim, arch[:2], max_archetypes=3, mdr=DEV)
    q = np.random.default_rng(4).standard_normal((2, dim)).astype(F)
    rows = dc.find_inputs(dim, 3, 65)[1]
    first_two = [d for d in deltas if d.archetype_id < 2]
    s2 = dc.lib_set(lib, first_two)

    def answers(s, ds, reg):
        n = len(ds)
        pairs = [(i, (i * 5 + 1) % n) for i in range(n)]
        return [(s.dot_dense(q), do.dot_dense_all(reg, ds, q)), (s.cosine_similarity_dense(q), do.cosine_dense_all(reg, ds, q)),
                (s.to_dense(), do.decode_all(reg, ds)), (s.magnitudes(), do.magnitudes(reg, ds)),
                (lib.dot_deltas_same_archetype(s, s, pairs)[0], do.pairs_all(reg, ds, ds, pairs)[0]),
                (lib.find_best_batch(rows)[1], reg.find_best_many(rows)[1]),
                (lib.encode_batch(rows, 0.5).deltas, do.pack([d for d, _ in reg.encode_batch(rows, 0.5)])["deltas"])]
    twin2 = do.ArchetypeRegistry(3)
    twin2.register(arch[0]), twin2.register(arch[1])
    before = answers(s2, first_two, twin2)
    assert all(dc.same(g, w) for g, w in before)
    # a register after the mirrors were made: the registry grows, the old set still answers as before, a new set sees three
    assert lib.register(arch[2]) == 2 and twin2.register(arch[2]) == 2
    s3 = dc.lib_set(lib, deltas)
    after3 = answers(s3, deltas, twin)
    assert all(dc.same(g, w) for g, w in after3)
    again = answers(s2, first_two, twin2)
    for (g0, _), (g1, w1) in zip(before[:5], again[:5]):
        assert dc.same(g0, g1) and dc.same(g1, w1)
    assert all(dc.same(g, w) for g, w in again[5:])                        # find_best and encode now see the third archetype
